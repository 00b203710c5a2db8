#!/usr/bin/env python3
"""Times awfmGpuScoreWindowsAffine on the 3.1 Gbp synthetic index bench.py uses, the text uploaded with awfmGpuIndexSetText.
Device events around every one of --steps calls after --warmup, the sides taking turns call by call in one process; spreads as
min / median / max.

  workload    --reads (2^20) reads of 150 characters cut from the text with 5 % substitutions, each with a window of 600
              positions that holds its locus at a random offset, in a record table of --records equal records.
  new call    awfmGpuScoreWindowsAffine with every output, scoring (1, 4, 6, 1), minScore 30, one slot column.
  comparator  (a) what a caller can do without it: ONE awfmGpuScoreChainsAffine call on 16 synthetic slots of 63 diagonals
              (w = 31, x = 0) that tile the window's diagonals -150 .. 600 with a stride of 47: more cells than the window has,
              and wrong whenever the path crosses a tile's edge -- the share of reads whose best score equals the new call's
              is reported; (b) the host twin on --threads (16) threads, wall clock, one call.
  bar         the new call's median lies below (a)'s by more than the sum of the two sides' max - min.
  parity      every output of the new call against awfmScoreWindowsAffine over the same arrays copied to the host, all reads,
              in the same run.
  efficiency  cells per second, and against the skew-and-padding ideal: a read of n rows in a window of W columns costs a wave
              (n + ceil(W / Q) - 1) steps of Q cells in each of 64 lanes, of which n W are cells of the window.

Prints one JSON line and writes it to --out (default profiles/window_scores/timing.json)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

READ_LENGTH, WIDTH, SCORING, MIN_SCORE = 150, 600, (1, 4, 6, 1), 30
TILES, TILE_PAD, TILE_STRIDE, FIRST_DIAGONAL = 16, 31, 47, -150 + 31


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
    p.add_argument("--out", default=os.path.join("profiles", "window_scores", "timing.json"))
    args = p.parse_args()

    import numpy as np
    import torch
    from avxwindowfmindex_amd import _lib, api
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream_obj = torch.cuda.Stream()
    stream = stream_obj.cuda_stream
    R, n, M, W = args.reads, args.text_len, READ_LENGTH, WIDTH
    result = {"reads": R, "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
              "parameters": {"read_length": M, "window": W, "records": args.records, "host_threads": args.threads, "scoring": list(SCORING),
                             "min_score": MIN_SCORE, "tiles": TILES, "tile_pad": TILE_PAD, "tile_stride": TILE_STRIDE}}

    # ---- the index, the text, the reads and their windows: all before the clock starts ----
    t0 = time.time()
    d_text = torch.empty(n, dtype=torch.uint8, device=dev)
    assert L.awfmGpuSynthText(d_text.data_ptr(), 0, n, 2, 0, None) == 1
    torch.cuda.synchronize()
    ix = api.gpu_create_index(d_text.data_ptr(), api.AwFmAlphabetDna, args.sa_ratio, args.seed_k, on_device_length=n, device=0)
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
    # a read lies inside one record, W positions from its ends: sequence-local loci
    record_length = n // args.records - 1
    d_sequence = torch.randint(0, args.records, (R,), device=dev, generator=gen)
    d_locus = torch.randint(W, record_length - W - M, (R,), device=dev, generator=gen)
    d_record_start = torch.from_numpy(np.concatenate(([0], host_ends[:-1].astype(np.int64) + 1))).to(dev)
    d_begin = d_locus - torch.randint(0, W - M + 1, (R,), device=dev, generator=gen)
    for begin in range(0, R, 1 << 18):
        r = min(1 << 18, R - begin)
        at = (d_record_start[d_sequence[begin:begin + r]] + d_locus[begin:begin + r]).unsqueeze(1)
        piece = d_text[at + torch.arange(M, device=dev)]
        swap = torch.rand((r, M), device=dev, generator=gen) < 0.05
        piece = torch.where(swap, letters[torch.randint(0, 4, (r, M), device=dev, generator=gen)], piece)
        d_reads[begin * M:(begin + r) * M] = piece.reshape(-1)
    del d_text
    torch.cuda.empty_cache()
    d_offsets = (torch.arange(R + 1, device=dev) * M).contiguous()
    d_window_sequences = d_sequence.to(torch.int32).contiguous()
    d_window_begins = d_begin.contiguous()
    d_window_ends = (d_begin + W).contiguous()

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
    costs = api.align_scoring(*SCORING)
    fields = (("scores", "int32"), ("readBegins", "int32"), ("readEnds", "int32"), ("textBegins", "int64"), ("textEnds", "int64"),
              ("sequences", "int32"), ("chainAnchors", "int32"), ("chainReadBegins", "int32"), ("chainReadEnds", "int32"),
              ("chainBeginDiagonals", "int64"), ("chainEndDiagonals", "int64"))
    new_out = {name: torch.zeros(R, dtype=getattr(torch, dtype), device=dev) for name, dtype in fields}
    d_counters = torch.zeros(2, dtype=torch.int64, device=dev)
    win = api.window_inputs(d_reads.data_ptr(), R * M, d_offsets.data_ptr(), d_window_sequences.data_ptr(), d_window_begins.data_ptr(),
                            d_window_ends.data_ptr())
    wout = api.window_score_outputs(numUnscored=d_counters.data_ptr(), numFound=d_counters.data_ptr() + 8,
                                    **{name: t.data_ptr() for name, t in new_out.items()})
    scratch_bytes = g.score_windows_affine_scratch_bytes(M)
    d_scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=dev)

    def new_call():
        g.score_windows_affine(win, R, wout, d_scratch.data_ptr(), M, scoring=costs, min_score=MIN_SCORE, stream=stream)

    # ---- comparator (a): sixteen synthetic slots that tile the window's diagonals ----
    tile = torch.arange(TILES, device=dev)
    diagonals = (d_begin.unsqueeze(1) + FIRST_DIAGONAL + TILE_STRIDE * tile).contiguous()  # sequence-local: t - i
    assert int(diagonals.min()) >= 0  # (a window begins at least 150 positions into its record: no tile begins before the record)
    tiles = {"sequences": d_window_sequences.unsqueeze(1).repeat(1, TILES).contiguous(),
             "chainAnchors": torch.ones((R, TILES), dtype=torch.int32, device=dev),
             "chainReadBegins": torch.zeros((R, TILES), dtype=torch.int32, device=dev),
             "chainReadEnds": torch.zeros((R, TILES), dtype=torch.int32, device=dev),
             "chainBeginDiagonals": diagonals, "chainEndDiagonals": diagonals.clone()}
    vin = api.verify_inputs(d_reads.data_ptr(), R * M, d_offsets.data_ptr(), **{name: t.data_ptr() for name, t in tiles.items()})
    tile_out = {"slotScores": torch.zeros(R * TILES, dtype=torch.int32, device=dev), "bestScores": torch.zeros(R, dtype=torch.int32, device=dev),
                "bestSlots": torch.zeros(R, dtype=torch.int32, device=dev)}
    sout = api.slot_score_outputs(**{name: t.data_ptr() for name, t in tile_out.items()})
    torch.cuda.synchronize()

    def tiled_call():
        g.score_chains_affine(vin, R, sout, max_candidates=TILES, band_pad=TILE_PAD, max_drift=0, scoring=costs, min_score=MIN_SCORE, mapq_cap=60,
                              stream=stream)

    ours, theirs = timed(new_call, tiled_call)

    # ---- parity and comparator (b): the host twin on the same arrays, all reads ----
    host = {name: t.cpu().numpy() for name, t in (("chars", d_reads[:R * M]), ("offsets", d_offsets), ("sequences", d_window_sequences),
                                                  ("begins", d_window_begins), ("ends", d_window_ends))}
    host_out = {name: np.zeros(R, getattr(np, dtype)) for name, dtype in fields}
    host_counters = np.zeros(2, np.uint64)
    hin = api.window_inputs(host["chars"].ctypes.data, R * M, host["offsets"].ctypes.data, host["sequences"].ctypes.data, host["begins"].ctypes.data,
                            host["ends"].ctypes.data)
    hout = api.window_score_outputs(numUnscored=host_counters.ctypes.data, numFound=host_counters.ctypes.data + 8,
                                    **{name: a.ctypes.data for name, a in host_out.items()})
    t = time.perf_counter()
    rc = L.awfmScoreWindowsAffine(C.byref(hin), R, C.byref(costs), MIN_SCORE, 1, 0, host_text.ctypes.data, n, host_ends.ctypes.data, args.records,
                                  api.AwFmAlphabetDna, C.byref(hout), args.threads)
    host_ms = (time.perf_counter() - t) * 1e3
    assert rc == _lib.AwFmSuccess, rc
    calls = args.steps + args.warmup
    got = {name: t.cpu().numpy() for name, t in new_out.items()}
    counters = d_counters.cpu().numpy()
    equal = {name: bool(np.array_equal(got[name], host_out[name])) for name in host_out}
    equal["numUnscored"] = int(counters[0]) == calls * int(host_counters[0])
    equal["numFound"] = int(counters[1]) == calls * int(host_counters[1])
    new_s, old_s = summary(ours), summary(theirs)
    spreads = (new_s["max_ms"] - new_s["min_ms"]) + (old_s["max_ms"] - old_s["min_ms"])
    scores = got["scores"].astype(np.int64) & 0xFFFFFFFF
    tiled_best = tile_out["bestScores"].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    counted = np.where(scores >= MIN_SCORE, scores, 0)
    at_locus = (got["textBegins"] <= (d_locus.cpu().numpy() + 10)) & (got["textEnds"] >= (d_locus.cpu().numpy() + M - 10))
    cells = R * M * W
    q = 12 if W > 512 else 8 if W > 256 else 4
    steps_cells = R * (M + -(-W // q) - 1) * q * 64
    result.update(new_call=new_s, tiled_score_chains_call=old_s, host_twin_ms=round(host_ms, 1), results_equal=all(equal.values()),
                  results_equal_by_output=equal, reads_compared=R, scratch_bytes=scratch_bytes, reads_found=int(host_counters[1]),
                  share_found_at_their_locus=round(float(at_locus.mean()), 5), mean_score=round(float(scores.mean()), 3),
                  share_tiled_best_equals_new=round(float((tiled_best == counted).mean()), 5), cells=cells,
                  cells_per_second=round(cells / (new_s["median_ms"] * 1e-3), 0), columns_per_lane=q,
                  ideal_share_of_lane_steps=round(cells / steps_cells, 4),
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
