#!/usr/bin/env python3
"""Times the end-bonus calls of slot scores and affine alignment (include/awfm_gpu.h, "end bonus") and counts what the bonus changes.
Device events around every one of --steps calls after --warmup, the sides taking turns call by call in one process; spreads as
min / median / max.  The script repeats scripts/matrix_scores_timing.py's preparation in its own text; it imports nothing from
it.  One preparation -- the batch of scripts/align_affine_timing.py: 2^20 reads of 150 characters, 5 % substitutions, the 3.1 Gbp
synthetic index, chains and verification's bestSlots on the device before the clock starts --, then three parts:

  siblings   awfmGpuAlignChainsAffine, awfmGpuScoreChainsAffine, awfmGpuAlignChainsMatrix and awfmGpuScoreChainsMatrix under
             (1, 4, 6, 1) resp. its uniform matrix, of this build and of --parent-lib, the library built from the parent commit:
             loaded beside this one with a handle of its own that binds the four calls alone, on the same image and arrays, the
             two builds taking turns call by call; every output compared over all reads.  Bar: the medians of the two builds
             differ by no more than the summed max - min of the two sides: the calls whose bodies gained the bonus policy must
             not have slowed down.  Left out without --parent-lib.
  bonus      each end-bonus call at B = 0 and at B = 5 against its matrix sibling of this build under the uniform (1, 4, 6, 1)
             matrix, the six calls taking turns; at B = 0 every output compared with the sibling's over all reads.  The ratio is
             an expectation (inside the spreads: one add and one select in one row per read), not a bar.
  clipped    awfmAlignChainsEndBonus, the host twin, on --threads threads over the same arrays copied to the host under B = 0 and
             B = 5: the reads clipped at one end or both under either, and the reads whose editDistances rose -- the
             substitutions that came back; the device's outputs under either B compared with the twin's over all reads.

Prints one JSON line and writes it to --out (default profiles/end_bonus/timing.json)."""
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
AFFINE_FIELDS = (("scores", "int32", 1), ("editDistances", "int32", 1), ("readBegins", "int32", 1), ("readEnds", "int32", 1), ("textBegins", "int64", 1),
                 ("textEnds", "int64", 1), ("numOps", "int32", 1), ("ops", "int32", MAX_OPS), ("numUnaligned", "int64", 0), ("numTruncated", "int64", 0))
SCORE_FIELDS = (("slotScores", "int32", SLOTS), ("slotReadEnds", "int32", SLOTS), ("slotTextEnds", "int64", SLOTS), ("bestSlots", "int32", 1),
                ("bestScores", "int32", 1), ("secondSlots", "int32", 1), ("secondScores", "int32", 1), ("mappingQualities", "uint8", 1),
                ("numUnscored", "int64", 0), ("numMapped", "int64", 0))


def count(text):
    return int(float(text))


def summary(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4), "calls": len(ms)}


def spread(s):
    return s["max_ms"] - s["min_ms"]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--parent-lib", default="", help="libawfmindex_amd.so built from the parent commit")
    p.add_argument("--text-len", type=count, default=3_100_000_000)
    p.add_argument("--reads", type=count, default=1 << 20)
    p.add_argument("--records", type=int, default=24)
    p.add_argument("--threads", type=int, default=16)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--bonus", type=int, default=5)
    p.add_argument("--out", default=os.path.join("profiles", "end_bonus", "timing.json"))
    args = p.parse_args()

    import numpy as np
    import torch
    from avxwindowfmindex_amd import _lib, api
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream_obj = torch.cuda.Stream()
    stream = stream_obj.cuda_stream
    R, M, n = args.reads, READ_LENGTH, args.text_len
    step, cap, min_length = STEP, CAP, MIN_LENGTH
    alphabet = api.AwFmAlphabetDna
    result = {"library": os.path.basename(_lib.LIB_PATH), "reads": R, "steps": args.steps, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0), "end_bonus": args.bonus,
              "parameters": {"read_length": M, "step": step, "cap": cap, "min_length": min_length, "max_hits_per_seed": MAX_HITS_PER_SEED, "band": BAND,
                             "min_votes": MIN_VOTES, "slots": SLOTS, "lookback": LOOKBACK, "gap_penalty": GAP_PENALTY, "records": args.records,
                             "host_threads": args.threads, "band_pad": BAND_PAD, "max_drift": MAX_DRIFT, "max_ops": MAX_OPS, "max_rows": M,
                             "text_length": n, "scoring": list(SCORING)}}

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

    # ---- the index, the reads, their seeds, located and mapped, clustered and chained: all before the clock starts ----
    t0 = time.time()
    d_text = torch.empty(n, dtype=torch.uint8, device=dev)
    assert L.awfmGpuSynthText(d_text.data_ptr(), 0, n, 2, 0, None) == 1
    torch.cuda.synchronize()
    ix = api.gpu_create_index(d_text.data_ptr(), alphabet, 8, 12, on_device_length=n, device=0)
    g = api.GpuIndex(ix, acquire=True)
    host_ends = np.array([(r + 1) * n // args.records - 1 for r in range(args.records)], np.uint64)
    g.set_record_table(host_ends)
    result["index_build_s"] = round(time.time() - t0, 2)
    host_text = d_text.cpu().numpy()
    torch.cuda.synchronize()
    g.set_text(host_text)

    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    d_reads = torch.empty(R * M + 64, dtype=torch.uint8, device=dev)
    letters = torch.tensor(list(b"acgt"), dtype=torch.uint8, device=dev)
    rate = 0.05
    for begin in range(0, R, 1 << 17):
        r = min(1 << 17, R - begin)
        at = torch.randint(0, n - M, (r, 1), device=dev, generator=gen)
        piece = d_text[at + torch.arange(M, device=dev)]
        swap = torch.rand((r, M), device=dev, generator=gen) < rate
        piece = torch.where(swap, letters[torch.randint(0, letters.numel(), (r, M), device=dev, generator=gen)], piece)
        d_reads[begin * M:(begin + r) * M] = piece.reshape(-1)
    del d_text
    torch.cuda.empty_cache()
    e = torch.arange(step, M + 1, step, device=dev)
    per_read = e.numel()
    base = (torch.arange(R, device=dev) * M).unsqueeze(1)
    d_ends = (base + e).reshape(-1).contiguous()
    d_starts = (base + torch.clamp(e - cap, min=0)).reshape(-1).contiguous()
    S = d_ends.numel()
    d_seed_ends = e.to(torch.int32).repeat(R).contiguous()
    d_read_offsets = (torch.arange(R + 1, device=dev) * per_read).contiguous()
    d_lengths = torch.empty(S, dtype=torch.int32, device=dev)
    d_ranges = torch.empty(S * 2, dtype=torch.int64, device=dev)
    d_counts = torch.empty(S, dtype=torch.int32, device=dev)
    d_hit_offsets = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    d_scan = torch.zeros(api.GpuIndex.scan_scratch_bytes(S), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    g.longest_suffix_matches(d_reads.data_ptr(), d_starts.data_ptr(), d_ends.data_ptr(), 0, S, min_length, d_lengths.data_ptr(),
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
    cand_out = {name: torch.empty(R * SLOTS, dtype=getattr(torch, dtype), device=dev) for name, dtype in CANDIDATE_FIELDS}
    d_scratch = torch.empty(max(api.read_candidates_scratch_bytes(R), api.read_chains_scratch_bytes(R)), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    g.read_candidates(cin, R, api.candidate_outputs(**{name: t.data_ptr() for name, t in cand_out.items()}), d_scratch.data_ptr(),
                      max_hits_per_seed=MAX_HITS_PER_SEED, band=BAND, min_votes=MIN_VOTES, max_candidates=SLOTS, stream=stream)
    stream_obj.synchronize()
    chain_out = {name: torch.empty(R * SLOTS, dtype=getattr(torch, dtype), device=dev) for name, dtype in CHAIN_FIELDS}
    g.read_chains(cin, R, cand_out["sequences"].data_ptr(), cand_out["diagonals"].data_ptr(), cand_out["diagonalSpans"].data_ptr(),
                  api.chain_outputs(**{name: t.data_ptr() for name, t in chain_out.items()}), d_scratch.data_ptr(), max_hits_per_seed=MAX_HITS_PER_SEED,
                  band=BAND, max_candidates=SLOTS, lookback=LOOKBACK, gap_penalty=GAP_PENALTY, stream=stream)
    stream_obj.synchronize()

    d_char_offsets = (torch.arange(R + 1, device=dev) * M).contiguous()
    slot_names = ("chainAnchors", "chainReadBegins", "chainReadEnds", "chainBeginDiagonals", "chainEndDiagonals")
    d_slots = dict({name: chain_out[name] for name in slot_names}, sequences=cand_out["sequences"])
    vin = api.verify_inputs(d_reads.data_ptr(), R * M, d_char_offsets.data_ptr(), **{name: t.data_ptr() for name, t in d_slots.items()})
    d_best = torch.empty(R, dtype=torch.int32, device=dev)
    # the slots the affine timing aligns: verification's best
    g.verify_chains(vin, R, api.verify_outputs(bestSlots=d_best.data_ptr()), max_candidates=SLOTS, band_pad=BAND_PAD, max_drift=MAX_DRIFT, stream=stream)
    stream_obj.synchronize()
    d_trace = torch.empty(g.align_chains_affine_scratch_bytes(M), dtype=torch.uint8, device=dev)

    def outputs(fields, make):
        arrays = {name: torch.zeros(max(R * per, 1), dtype=getattr(torch, dtype), device=dev) for name, dtype, per in fields}
        return arrays, make(**{name: t.data_ptr() for name, t in arrays.items()})

    def same(got, want, fields):
        """every output over all reads; the rows of ops up to each read's numOps, truncated rows not at all"""
        equal = {}
        for name, _, per in fields:
            a = got[name].cpu().numpy() if hasattr(got[name], "cpu") else got[name]
            b = want[name].cpu().numpy() if hasattr(want[name], "cpu") else want[name]
            if name == "ops":
                counts = (got["numOps"].cpu().numpy() if hasattr(got["numOps"], "cpu") else got["numOps"]).astype(np.int64)
                live = (np.arange(MAX_OPS)[None, :] < counts[:, None]) & (counts[:, None] <= MAX_OPS)
                equal[name] = bool(np.array_equal(a.reshape(R, MAX_OPS)[live], b.reshape(R, MAX_OPS)[live]))
            else:
                equal[name] = bool(np.array_equal(a, b))
        return equal

    costs = api.align_scoring(*SCORING)
    uniform = api.matrix_scoring_uniform(alphabet, SCORING)

    def device_calls(lib):
        """the four existing calls of a library on the same image and arrays -> ([fn, ...], [outputs, ...], [fields, ...])"""
        outs = [outputs(AFFINE_FIELDS, api.affine_outputs), outputs(SCORE_FIELDS, api.slot_score_outputs), outputs(AFFINE_FIELDS, api.affine_outputs),
                outputs(SCORE_FIELDS, api.slot_score_outputs)]

        def align(symbol, scoring, out):
            def fn():
                assert getattr(lib, symbol)(g.handle, C.byref(vin), d_best.data_ptr(), R, SLOTS, BAND_PAD, MAX_DRIFT, C.byref(scoring), MAX_OPS, M,
                                            C.byref(out), d_trace.data_ptr(), stream) == _lib.AwFmSuccess
            return fn

        def score(symbol, scoring, out):
            def fn():
                assert getattr(lib, symbol)(g.handle, C.byref(vin), R, SLOTS, BAND_PAD, MAX_DRIFT, C.byref(scoring), 0, 60, C.byref(out), stream) == _lib.AwFmSuccess
            return fn

        fns = [align("awfmGpuAlignChainsAffine", costs, outs[0][1]), score("awfmGpuScoreChainsAffine", costs, outs[1][1]),
               align("awfmGpuAlignChainsMatrix", uniform, outs[2][1]), score("awfmGpuScoreChainsMatrix", uniform, outs[3][1])]
        return fns, [o[0] for o in outs], [AFFINE_FIELDS, SCORE_FIELDS, AFFINE_FIELDS, SCORE_FIELDS]

    names = ("align_affine", "score_affine", "align_matrix", "score_matrix")
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))  # the four calls alone: the parent's library has no end-bonus calls to bind
        align_types = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                       C.c_void_p, C.c_void_p]
        score_types = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        for symbol, types in (("awfmGpuAlignChainsAffine", align_types), ("awfmGpuScoreChainsAffine", score_types), ("awfmGpuAlignChainsMatrix", align_types),
                              ("awfmGpuScoreChainsMatrix", score_types)):
            getattr(parent, symbol).restype, getattr(parent, symbol).argtypes = C.c_int, types
        this_fns, this_outs, fields = device_calls(L)
        parent_fns, parent_outs, _ = device_calls(parent)
        times = [summary(ms) for ms in timed(*[fn for pair in zip(this_fns, parent_fns) for fn in pair])]
        equal = {name: same(this_outs[k], parent_outs[k], fields[k]) for k, name in enumerate(names)}
        result["siblings"] = dict({name: {"this": times[2 * k], "parent": times[2 * k + 1]} for k, name in enumerate(names)},
                                  results_equal_by_output=equal, results_equal=all(all(v.values()) for v in equal.values()), reads_compared=R,
                                  bar={name: {"this_minus_parent_ms": round(times[2 * k]["median_ms"] - times[2 * k + 1]["median_ms"], 4),
                                              "summed_spreads_ms": round(spread(times[2 * k]) + spread(times[2 * k + 1]), 4),
                                              "met": bool(abs(times[2 * k]["median_ms"] - times[2 * k + 1]["median_ms"]) <=
                                                          spread(times[2 * k]) + spread(times[2 * k + 1]))} for k, name in enumerate(names)})
        del this_outs, parent_outs, this_fns, parent_fns
        torch.cuda.empty_cache()

    # ---- the end-bonus calls at B = 0 and B = --bonus against the matrix siblings of this build ----
    sibling_fns, sibling_outs, _ = device_calls(L)
    bonus_outs = {}

    def align_bonus(B):
        arrays, out = outputs(AFFINE_FIELDS, api.affine_outputs)
        bonus_outs["align", B] = arrays

        def fn():
            g.align_chains_end_bonus(vin, d_best.data_ptr(), R, out, d_trace.data_ptr(), max_candidates=SLOTS, band_pad=BAND_PAD, max_drift=MAX_DRIFT,
                                     scoring=uniform, end_bonus=B, max_ops=MAX_OPS, max_rows=M, stream=stream)
        return fn

    def score_bonus(B):
        arrays, out = outputs(SCORE_FIELDS, api.slot_score_outputs)
        bonus_outs["score", B] = arrays

        def fn():
            g.score_chains_end_bonus(vin, R, out, max_candidates=SLOTS, band_pad=BAND_PAD, max_drift=MAX_DRIFT, scoring=uniform, end_bonus=B, stream=stream)
        return fn

    times = [summary(ms) for ms in timed(sibling_fns[2], align_bonus(0), align_bonus(args.bonus), sibling_fns[3], score_bonus(0), score_bonus(args.bonus))]
    equal = {"align": same(bonus_outs["align", 0], sibling_outs[2], AFFINE_FIELDS), "score": same(bonus_outs["score", 0], sibling_outs[3], SCORE_FIELDS)}
    result["bonus"] = dict(align_matrix=times[0], align_end_bonus_0=times[1], align_end_bonus=times[2], score_matrix=times[3], score_end_bonus_0=times[4],
                           score_end_bonus=times[5], no_bonus_equals_matrix_by_output=equal,
                           no_bonus_equals_matrix=all(all(v.values()) for v in equal.values()), reads_compared=R,
                           ratio={f"{call}_{label}_over_matrix": round(times[k + d]["median_ms"] / times[k]["median_ms"], 4)
                                  for call, k in (("align", 0), ("score", 3)) for label, d in (("end_bonus_0", 1), ("end_bonus", 2))},
                           difference_ms={f"{call}_{label}": round(times[k + d]["median_ms"] - times[k]["median_ms"], 4)
                                          for call, k in (("align", 0), ("score", 3)) for label, d in (("end_bonus_0", 1), ("end_bonus", 2))},
                           summed_spreads_ms={f"{call}_{label}": round(spread(times[k + d]) + spread(times[k]), 4)
                                              for call, k in (("align", 0), ("score", 3)) for label, d in (("end_bonus_0", 1), ("end_bonus", 2))})

    # ---- what the bonus changes, counted from the host twin's outputs over all reads; the device is compared with it ----
    host_chars, host_offsets = d_reads[:R * M].cpu().numpy(), d_char_offsets.cpu().numpy()
    host_slots = {name: t.cpu().numpy() for name, t in d_slots.items()}
    host_best = d_best.cpu().numpy()
    hin = api.verify_inputs(host_chars.ctypes.data, R * M, host_offsets.ctypes.data, **{name: a.ctypes.data for name, a in host_slots.items()})
    clipped, twin = {}, {}
    for B in (0, args.bonus):
        host_align = {name: np.zeros(max(R * per, 1), getattr(np, dtype)) for name, dtype, per in AFFINE_FIELDS}
        haout = api.affine_outputs(**{name: a.ctypes.data for name, a in host_align.items()})
        t = time.perf_counter()
        rc = L.awfmAlignChainsEndBonus(C.byref(hin), host_best.ctypes.data, R, SLOTS, BAND_PAD, MAX_DRIFT, C.byref(uniform), B, MAX_OPS, host_text.ctypes.data, n,
                                       host_ends.ctypes.data, args.records, alphabet, C.byref(haout), args.threads)
        assert rc == _lib.AwFmSuccess, rc
        seconds = time.perf_counter() - t
        twin[B] = host_align
        scores = host_align["scores"].astype(np.int64) & 0xFFFFFFFF
        aligned = (scores > 0) & (scores < 0xFFFFFFFC)
        left, right = aligned & (host_align["readBegins"] > 0), aligned & (host_align["readEnds"].astype(np.int64) < M)
        for name in ("numUnaligned", "numTruncated"):  # the device's counters were added to by every call, warm-up included
            total = int(bonus_outs["align", B][name].item())
            assert total % (args.steps + args.warmup) == 0, (name, total)
            bonus_outs["align", B][name].fill_(total // (args.steps + args.warmup))
        equal = same(bonus_outs["align", B], host_align, AFFINE_FIELDS)
        clipped[str(B)] = {"reads_aligned": int(aligned.sum()), "clipped_at_the_start": int(left.sum()), "clipped_at_the_end": int(right.sum()),
                           "clipped_at_one_end_or_both": int((left | right).sum()), "share_clipped": round(float((left | right).sum()) / R, 5),
                           "mean_score": round(float(scores[aligned].mean()), 3), "edit_characters": int(host_align["editDistances"][aligned].sum()),
                           "truncated": int(host_align["numTruncated"][0]), "host_twin_s": round(seconds, 3), "device_equals_host_twin_by_output": equal,
                           "device_equals_host_twin": all(equal.values())}
    rose = twin[args.bonus]["editDistances"].astype(np.int64) - twin[0]["editDistances"].astype(np.int64)
    result["clipped"] = dict(clipped, reads=R, reads_whose_edit_distance_rose=int((rose > 0).sum()), edit_characters_that_came_back=int(rose[rose > 0].sum()),
                             reads_whose_edit_distance_fell=int((rose < 0).sum()))

    text = json.dumps(result)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
