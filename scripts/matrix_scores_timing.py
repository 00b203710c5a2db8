#!/usr/bin/env python3
"""Times the matrix twins of slot scores and affine alignment (include/awfm_gpu.h, "substitution matrices").  Device events around
every one of --steps calls after --warmup, the sides taking turns call by call in one process; spreads as min / median / max.
The script repeats scripts/align_affine_timing.py's preparation in its own text; it imports nothing from it.

  --leg siblings   the batch of scripts/align_affine_timing.py (2^20 reads of 150 characters, 5 % substitutions, the 3.1 Gbp
                   synthetic index, chains and verification's bestSlots on the device before the clock starts);
                   awfmGpuScoreChainsAffine and awfmGpuAlignChainsAffine under (1, 4, 6, 1), of this build and of --parent-lib,
                   the library built from the parent commit: loaded beside this one with a handle of its own that binds the two
                   calls alone, on the same image and arrays, the two builds taking turns call by call; every output compared
                   over all reads.  Bar: the medians of the two builds differ by no more than the summed max - min of the two
                   sides: the calls that exist on both sides must not have slowed down.
  --leg matrix     the same batch; each matrix call under awfmMatrixScoringUniform's (1, 4, 6, 1) matrix against its affine
                   sibling, the four calls taking turns; every output compared over all reads.  The ratio is an expectation
                   (near 1: one LDS byte load per cell instead of a select), not a bar.
  --leg protein    a synthetic amino text of the size bench.py uses for its amino leg (2e8 residues), --peptides (2^18) peptides
                   of 300 residues cut from it with 20 % substitutions; the longest match ending at every 2nd position, cap 32,
                   minLength 7; located, mapped, clustered and chained before the clock starts.  A matrix over -4..11, gaps
                   (11, 1).  awfmGpuScoreChainsMatrix and awfmGpuAlignChainsMatrix (on the score call's bestSlots) against their
                   host twins on --threads (16) threads over the same arrays copied to the host, wall clock; every output compared
                   over all reads.  Bar: each device median lies below its twin's by more than the summed max - min.
  --combine A B .. the legs' JSON files -> --out (default profiles/matrix_scores/timing.json), each under its leg's name.

Every leg prints one JSON line and writes it to --out."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

READ_LENGTH, STEP, CAP, MIN_LENGTH, MAX_HITS_PER_SEED, BAND, MIN_VOTES, SLOTS, LOOKBACK, GAP_PENALTY = 150, 4, 64, 16, 32, 8, 2, 4, 64, 1
BAND_PAD, MAX_DRIFT, MAX_OPS, SCORING = 8, 15, 32, (1, 4, 6, 1)
PEPTIDE_LENGTH, PEPTIDE_STEP, PEPTIDE_CAP, PEPTIDE_MIN_LENGTH, PEPTIDE_RATE, PEPTIDE_GAPS = 300, 2, 32, 7, 0.20, (11, 1)
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


def combine(paths, out):
    legs = [json.load(open(path)) for path in paths]
    result = dict({"device": legs[0].get("device")}, **{leg["leg"]: leg for leg in legs})
    text = json.dumps(result)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text + "\n")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--leg", choices=["siblings", "matrix", "protein"])
    p.add_argument("--parent-lib", default="", help="siblings: libawfmindex_amd.so built from the parent commit")
    p.add_argument("--combine", nargs="+")
    p.add_argument("--text-len", type=count, default=None, help="default 3.1e9 (nucleotide legs) / 2e8 (protein)")
    p.add_argument("--reads", type=count, default=1 << 20)
    p.add_argument("--peptides", type=count, default=1 << 18)
    p.add_argument("--records", type=int, default=24)
    p.add_argument("--threads", type=int, default=16)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--out", default=os.path.join("profiles", "matrix_scores", "timing.json"))
    args = p.parse_args()
    if args.combine:
        return combine(args.combine, args.out)

    import numpy as np
    import torch
    from avxwindowfmindex_amd import _lib, api
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream_obj = torch.cuda.Stream()
    stream = stream_obj.cuda_stream
    protein = args.leg == "protein"
    R, M = (args.peptides, PEPTIDE_LENGTH) if protein else (args.reads, READ_LENGTH)
    n = args.text_len or (200_000_000 if protein else 3_100_000_000)
    step, cap, min_length = (PEPTIDE_STEP, PEPTIDE_CAP, PEPTIDE_MIN_LENGTH) if protein else (STEP, CAP, MIN_LENGTH)
    alphabet = api.AwFmAlphabetAmino if protein else api.AwFmAlphabetDna
    result = {"leg": args.leg, "library": os.path.basename(_lib.LIB_PATH), "reads": R, "steps": args.steps, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0),
              "parameters": {"read_length": M, "step": step, "cap": cap, "min_length": min_length, "max_hits_per_seed": MAX_HITS_PER_SEED, "band": BAND,
                             "min_votes": MIN_VOTES, "slots": SLOTS, "lookback": LOOKBACK, "gap_penalty": GAP_PENALTY, "records": args.records,
                             "host_threads": args.threads, "band_pad": BAND_PAD, "max_drift": MAX_DRIFT, "max_ops": MAX_OPS, "max_rows": M,
                             "text_length": n}}

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
    assert L.awfmGpuSynthText(d_text.data_ptr(), 0, n, 4 if protein else 2, 1 if protein else 0, None) == 1
    torch.cuda.synchronize()
    ix = api.gpu_create_index(d_text.data_ptr(), alphabet, 8, 5 if protein else 12, on_device_length=n, device=0)
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
    letters = torch.tensor(list(b"acdefghiklmnpqrstvwy" if protein else b"acgt"), dtype=torch.uint8, device=dev)
    rate = PEPTIDE_RATE if protein else 0.05
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
    if not protein:  # the slots the affine timing aligns: verification's best
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
    if not protein:
        affine_out, aout = outputs(AFFINE_FIELDS, api.affine_outputs)
        score_out, sout = outputs(SCORE_FIELDS, api.slot_score_outputs)

        def align_affine():
            g.align_chains_affine(vin, d_best.data_ptr(), R, aout, d_trace.data_ptr(), max_candidates=SLOTS, band_pad=BAND_PAD, max_drift=MAX_DRIFT,
                                  scoring=costs, max_ops=MAX_OPS, max_rows=M, stream=stream)

        def score_affine():
            g.score_chains_affine(vin, R, sout, max_candidates=SLOTS, band_pad=BAND_PAD, max_drift=MAX_DRIFT, scoring=costs, stream=stream)

        if args.leg == "siblings":
            if not args.parent_lib:
                sys.exit("--leg siblings needs --parent-lib")
            parent = C.CDLL(os.path.abspath(args.parent_lib))  # the two calls alone: the parent's library has no matrix calls to bind
            parent.awfmGpuAlignChainsAffine.restype = parent.awfmGpuScoreChainsAffine.restype = C.c_int
            parent.awfmGpuAlignChainsAffine.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                                        C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
            parent.awfmGpuScoreChainsAffine.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32,
                                                        C.c_uint32, C.c_void_p, C.c_void_p]
            parent_affine_out, paout = outputs(AFFINE_FIELDS, api.affine_outputs)
            parent_score_out, psout = outputs(SCORE_FIELDS, api.slot_score_outputs)

            def align_parent():
                assert parent.awfmGpuAlignChainsAffine(g.handle, C.byref(vin), d_best.data_ptr(), R, SLOTS, BAND_PAD, MAX_DRIFT, C.byref(costs), MAX_OPS, M,
                                                       C.byref(paout), d_trace.data_ptr(), stream) == _lib.AwFmSuccess

            def score_parent():
                assert parent.awfmGpuScoreChainsAffine(g.handle, C.byref(vin), R, SLOTS, BAND_PAD, MAX_DRIFT, C.byref(costs), 0, 60, C.byref(psout),
                                                       stream) == _lib.AwFmSuccess

            times = [summary(ms) for ms in timed(align_affine, align_parent, score_affine, score_parent)]
            equal = {"align": same(affine_out, parent_affine_out, AFFINE_FIELDS), "score": same(score_out, parent_score_out, SCORE_FIELDS)}
            result.update(align_affine={"this": times[0], "parent": times[1]}, score_affine={"this": times[2], "parent": times[3]},
                          results_equal_by_output=equal, results_equal=all(all(v.values()) for v in equal.values()), reads_compared=R,
                          bar={call: {"this_minus_parent_ms": round(times[k]["median_ms"] - times[k + 1]["median_ms"], 4),
                                      "summed_spreads_ms": round(spread(times[k]) + spread(times[k + 1]), 4),
                                      "met": bool(abs(times[k]["median_ms"] - times[k + 1]["median_ms"]) <= spread(times[k]) + spread(times[k + 1]))}
                               for call, k in (("align_affine", 0), ("score_affine", 2))})
        else:
            uniform = api.matrix_scoring_uniform(alphabet, SCORING)
            matrix_out, mout = outputs(AFFINE_FIELDS, api.affine_outputs)
            matrix_score_out, msout = outputs(SCORE_FIELDS, api.slot_score_outputs)

            def align_matrix():
                g.align_chains_matrix(vin, d_best.data_ptr(), R, mout, d_trace.data_ptr(), max_candidates=SLOTS, band_pad=BAND_PAD, max_drift=MAX_DRIFT,
                                      scoring=uniform, max_ops=MAX_OPS, max_rows=M, stream=stream)

            def score_matrix():
                g.score_chains_matrix(vin, R, msout, max_candidates=SLOTS, band_pad=BAND_PAD, max_drift=MAX_DRIFT, scoring=uniform, stream=stream)

            times = [summary(ms) for ms in timed(align_affine, align_matrix, score_affine, score_matrix)]
            equal = {"align": same(matrix_out, affine_out, AFFINE_FIELDS), "score": same(matrix_score_out, score_out, SCORE_FIELDS)}
            result.update(align_affine=times[0], align_matrix=times[1], score_affine=times[2], score_matrix=times[3], results_equal_by_output=equal,
                          results_equal=all(all(v.values()) for v in equal.values()), reads_compared=R,
                          ratio={"align_matrix_over_affine": round(times[1]["median_ms"] / times[0]["median_ms"], 4),
                                 "align_summed_spreads_ms": round(spread(times[0]) + spread(times[1]), 4),
                                 "align_difference_ms": round(times[1]["median_ms"] - times[0]["median_ms"], 4),
                                 "score_matrix_over_affine": round(times[3]["median_ms"] / times[2]["median_ms"], 4),
                                 "score_summed_spreads_ms": round(spread(times[2]) + spread(times[3]), 4),
                                 "score_difference_ms": round(times[3]["median_ms"] - times[2]["median_ms"], 4)})
    else:
        rng = np.random.default_rng(7)
        values = rng.integers(-4, 12, (21, 21))
        values[np.arange(20), np.arange(20)] = rng.integers(4, 12, 20)
        matrix = api.matrix_scoring(values, *PEPTIDE_GAPS)
        score_out, sout = outputs(SCORE_FIELDS, api.slot_score_outputs)
        align_out, aout = outputs(AFFINE_FIELDS, api.affine_outputs)

        def score_matrix():
            g.score_chains_matrix(vin, R, sout, max_candidates=SLOTS, band_pad=BAND_PAD, max_drift=MAX_DRIFT, scoring=matrix, min_score=1, stream=stream)

        score_matrix()
        stream_obj.synchronize()
        d_best.copy_(score_out["bestSlots"])

        def align_matrix():
            g.align_chains_matrix(vin, d_best.data_ptr(), R, aout, d_trace.data_ptr(), max_candidates=SLOTS, band_pad=BAND_PAD, max_drift=MAX_DRIFT,
                                  scoring=matrix, max_ops=MAX_OPS, max_rows=M, stream=stream)

        host_chars, host_offsets = d_reads[:R * M].cpu().numpy(), d_char_offsets.cpu().numpy()
        host_slots = {name: t.cpu().numpy() for name, t in d_slots.items()}
        host_best = d_best.cpu().numpy()
        hin = api.verify_inputs(host_chars.ctypes.data, R * M, host_offsets.ctypes.data, **{name: a.ctypes.data for name, a in host_slots.items()})
        host_score = {name: np.zeros(max(R * per, 1), getattr(np, dtype)) for name, dtype, per in SCORE_FIELDS}
        host_align = {name: np.zeros(max(R * per, 1), getattr(np, dtype)) for name, dtype, per in AFFINE_FIELDS}
        hsout = api.slot_score_outputs(**{name: a.ctypes.data for name, a in host_score.items()})
        haout = api.affine_outputs(**{name: a.ctypes.data for name, a in host_align.items()})

        def host_score_twin():
            rc = L.awfmScoreChainsMatrix(C.byref(hin), R, SLOTS, BAND_PAD, MAX_DRIFT, C.byref(matrix), 1, 60, host_text.ctypes.data, n, host_ends.ctypes.data,
                                         args.records, alphabet, C.byref(hsout), args.threads)
            assert rc == _lib.AwFmSuccess, rc

        def host_align_twin():
            rc = L.awfmAlignChainsMatrix(C.byref(hin), host_best.ctypes.data, R, SLOTS, BAND_PAD, MAX_DRIFT, C.byref(matrix), MAX_OPS, host_text.ctypes.data, n,
                                         host_ends.ctypes.data, args.records, alphabet, C.byref(haout), args.threads)
            assert rc == _lib.AwFmSuccess, rc

        for name in ("numUnscored", "numMapped"):
            score_out[name].zero_()
        times = [summary(ms) for ms in timed(score_matrix, host_score_twin, align_matrix, host_align_twin, host=(host_score_twin, host_align_twin))]
        equal = {"score": same(score_out, host_score, SCORE_FIELDS), "align": same(align_out, host_align, AFFINE_FIELDS)}
        scores = align_out["scores"].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        aligned = (scores > 0) & (scores < 0xFFFFFFFC)
        result.update(score_matrix=times[0], score_host_twin=times[1], align_matrix=times[2], align_host_twin=times[3], results_equal_by_output=equal,
                      results_equal=all(all(v.values()) for v in equal.values()), reads_compared=R, reads_aligned=int(aligned.sum()),
                      mean_score=round(float(scores[aligned].mean()), 3) if aligned.any() else 0.0,
                      reads_mapped=int(score_out["numMapped"].item()) // (args.steps + args.warmup), matrix_range=[-4, 11], gaps=list(PEPTIDE_GAPS),
                      bar={call: {"summed_spreads_ms": round(spread(times[k]) + spread(times[k + 1]), 4),
                                  "speedup": round(times[k + 1]["median_ms"] / times[k]["median_ms"], 3),
                                  "met": bool(times[k + 1]["median_ms"] - times[k]["median_ms"] > spread(times[k]) + spread(times[k + 1]))}
                           for call, k in (("score", 0), ("align", 2))})

    text = json.dumps(result)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
