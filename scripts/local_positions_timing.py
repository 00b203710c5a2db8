#!/usr/bin/env python3
"""Times the mapping of located hits to sequence coordinates (awfmGpuLocalPositions) on the device, for 10^8 positions resident
there, `--steps` launches after `--warmup`, device time by events:

  1. the pass on genome-shaped tables (R = 25 and R = 640 over the index's positions, installed with set_record_table on the
     index bench.py builds; positions = the planted batch's located hits): the LDS lookup;
  2. the pass on a protein-shaped table (R = 5.7 * 10^5 records of about 360 residues; positions uniformly random below the last
     end, made on the device): the directory in memory;
  3. the floor both are judged against: a device-to-device copy of 10 bytes per position (10 read + 10 written = the pass's
     8 + 12 bytes of traffic), in the same process;
  4. the path the pass replaces: download of the positions to page-locked host memory + awfmLocalPositions on --host-threads
     threads (wall time);
  5. the planted located step (search in order, hit offsets, locate) with and without the pass appended.

Prints one JSON line and writes it to --out.  --no-index skips what needs the large index (1 on located hits, 5): the tables are
then installed on a small index and 1 runs on uniformly random positions.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def count(text):
    return int(float(text))


def genome_ends(records, positions, seed):
    """`records` records of unequal lengths (a few large ones, many small: exponential shares) that fill `positions` positions"""
    rng = np.random.default_rng(seed)
    share = rng.exponential(1.0, records) * np.where(np.arange(records) < 25, 40.0, 1.0)
    lengths = np.maximum((share / share.sum() * (positions - records - 1)).astype(np.uint64), 1)
    return (np.cumsum(lengths) + np.arange(records, dtype=np.uint64)).astype(np.uint64)


def protein_ends(records, seed):
    lengths = np.random.default_rng(seed).integers(50, 671, records).astype(np.uint64)  # 360 on average
    return (np.cumsum(lengths) + np.arange(records, dtype=np.uint64)).astype(np.uint64)


def summary(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4), "launches": len(ms)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--text-len", type=count, default=3_100_000_000)
    p.add_argument("--queries", type=count, default=100_000_000)
    p.add_argument("--kmer", type=int, default=21)
    p.add_argument("--seed-k", type=int, default=12)
    p.add_argument("--sa-ratio", type=int, default=8)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--host-threads", type=int, default=16)
    p.add_argument("--no-index", action="store_true")
    p.add_argument("--out", default=None)
    args = p.parse_args()

    import torch
    from avxwindowfmindex_amd import _lib, api
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream_obj = torch.cuda.Stream()
    stream = stream_obj.cuda_stream
    N, K = args.queries, args.kmer
    result = {"positions": N, "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}

    def timed(fn):
        """device ms of every one of --steps launches of fn on the stream, after --warmup"""
        for _ in range(args.warmup):
            fn()
        stream_obj.synchronize()
        out = []
        for _ in range(args.steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream_obj)
            fn()
            b.record(stream_obj)
            stream_obj.synchronize()
            out.append(a.elapsed_time(b))
        return out

    # ---- the index and the planted batch's located hits ----
    d_seq = torch.empty(N + 1024, dtype=torch.int32, device=dev)
    d_local = torch.empty(N + 1024, dtype=torch.int64, device=dev)
    d_illegal = torch.zeros(1, dtype=torch.int64, device=dev)
    if args.no_index:
        ix = api.create_index(np.frombuffer(b"acgtacgtacgtacgt" * 8, np.uint8), api.AwFmAlphabetDna, 2, 2)
        g = api.GpuIndex(ix)
        span = args.text_len
        d_pos = torch.randint(0, span, (N,), dtype=torch.int64, device=dev)
        hits = N
        step = None
    else:
        n = args.text_len
        t0 = time.time()
        d_text = torch.empty(n, dtype=torch.uint8, device=dev)
        assert L.awfmGpuSynthText(d_text.data_ptr(), 0, n, 2, 0, None) == 1
        torch.cuda.synchronize()
        ix = api.gpu_create_index(d_text.data_ptr(), api.AwFmAlphabetDna, args.sa_ratio, args.seed_k, on_device_length=n, device=0)
        g = api.GpuIndex(ix, acquire=True)
        result["index_build_s"] = round(time.time() - t0, 2)
        d_chars = torch.empty(N * K, dtype=torch.uint8, device=dev)
        assert L.awfmGpuSynthPlantedQueries(d_chars.data_ptr(), 0, N, K, 103, d_text.data_ptr(), n, None) == 1
        del d_text
        d_kmers = torch.empty(N, dtype=torch.int32, device=dev)
        d_ranges = torch.empty(N * 2, dtype=torch.int64, device=dev)
        d_counts = torch.empty(N, dtype=torch.int32, device=dev)
        d_off = torch.zeros(N + 1, dtype=torch.int64, device=dev)
        d_scratch = torch.empty(api.GpuIndex.scan_scratch_bytes(N), dtype=torch.uint8, device=dev)
        d_pos = torch.empty(N + N // 8 + 1024, dtype=torch.int64, device=dev)
        assert g.search_hits_is_ordered(False, K, N), "the planted step of the headline takes the seed-order path"

        def step(with_pass):
            g.search_hits_in_order(d_chars.data_ptr(), 0, K, N, d_kmers.data_ptr(), d_ranges.data_ptr(), stream=stream,
                                   d_order_counts=d_counts.data_ptr())
            g.hit_offsets_on_device(d_counts.data_ptr(), 0, N, d_off.data_ptr(), d_scratch.data_ptr(), stream)
            g.locate_on_device(d_ranges.data_ptr(), d_off.data_ptr(), N, d_pos.numel(), d_pos.data_ptr(), stream)
            if with_pass:
                g.local_positions(d_pos.data_ptr(), min(d_pos.numel(), d_local.numel()), d_seq.data_ptr(), d_local.data_ptr(),
                                  d_off.data_ptr() + 8 * N, d_illegal.data_ptr(), stream)

        step(False)
        stream_obj.synchronize()
        hits = int(d_off[N].item())
        span = n
        result["located_hits"] = hits
        hits = min(hits, d_local.numel())
    result["mapped_per_launch"] = hits

    def the_pass():
        g.local_positions(d_pos.data_ptr(), hits, d_seq.data_ptr(), d_local.data_ptr(), 0, d_illegal.data_ptr(), stream)

    # ---- 3. the floor: a device-to-device copy of 10 bytes per position ----
    d_a = torch.empty(hits * 10, dtype=torch.uint8, device=dev)
    d_b = torch.empty(hits * 10, dtype=torch.uint8, device=dev)
    d_a.fill_(1)

    def the_copy():
        with torch.cuda.stream(stream_obj):
            d_b.copy_(d_a, non_blocking=True)

    result["copy_10B_per_position"] = summary(timed(the_copy))
    floor = result["copy_10B_per_position"]["median_ms"]
    del d_a, d_b

    # ---- 1. genome-shaped tables: the LDS lookup ----
    for records in (25, 640):
        ends = genome_ends(records, span, records)
        g.set_record_table(ends)
        assert "lookup lds" in g.describe(), g.describe()
        entry = summary(timed(the_pass))
        entry["ratio_to_copy"] = round(entry["median_ms"] / floor, 3)
        entry["describe"] = g.describe().split("record table: ")[1].split(";")[0]
        result[f"pass_genome_R{records}"] = entry
    result["acceptance_1_at_most_1.5x_copy"] = bool(max(result["pass_genome_R25"]["ratio_to_copy"], result["pass_genome_R640"]["ratio_to_copy"]) <= 1.5)

    # ---- 4. the path it replaces: download + awfmLocalPositions on the host (on the R = 640 table) ----
    fa_ends = genome_ends(640, span, 640)
    host_ix = host_index_with_table(api, fa_ends)
    pinned = torch.empty(hits, dtype=torch.int64).pin_memory()
    host_seq = np.zeros(hits, np.uint32)
    host_local = np.zeros(hits, np.uint64)
    torch.cuda.synchronize()
    downloads, maps = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        pinned.copy_(d_pos[:hits], non_blocking=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        _, _, host_illegal = api.local_positions_host(host_ix, pinned.numpy().view(np.uint64), threads=args.host_threads,
                                                      out_sequence=host_seq, out_local=host_local)
        t2 = time.perf_counter()
        downloads.append((t1 - t0) * 1e3)
        maps.append((t2 - t1) * 1e3)
    result["host_path_genome_R640"] = {"download_ms": round(min(downloads), 2), "map_ms": round(min(maps), 2),
                                       "total_ms": round(min(downloads) + min(maps), 2), "threads": args.host_threads}
    # (and the device pass on that table gives what the host gives)
    d_illegal.zero_()
    the_pass()
    stream_obj.synchronize()
    assert int(d_illegal.item()) == host_illegal
    assert np.array_equal(d_seq[:hits].cpu().numpy().view(np.uint32), host_seq)
    assert np.array_equal(d_local[:hits].cpu().numpy().view(np.uint64), host_local)
    result["device_equals_host_on_R640"] = True
    host_ix.dealloc()

    # ---- 5. the planted located step with and without the pass ----
    if step is not None:
        without = summary(timed(lambda: step(False)))
        with_pass = summary(timed(lambda: step(True)))
        result["planted_step"] = {"without_pass": without, "with_pass": with_pass,
                                  "difference_ms": round(with_pass["median_ms"] - without["median_ms"], 4)}

    # ---- 2. a protein-shaped table: the directory in memory ----
    ends = protein_ends(570_000, 57)
    g.set_record_table(ends)
    assert "lookup dir" in g.describe(), g.describe()
    d_pos = None
    d_pos = torch.randint(0, int(ends[-1]), (hits,), dtype=torch.int64, device=dev)
    entry = summary(timed(the_pass))
    entry["ratio_to_copy"] = round(entry["median_ms"] / floor, 3)
    entry["describe"] = g.describe().split("record table: ")[1].split(";")[0]
    entry["text_positions"] = int(ends[-1])
    result["pass_protein_R570000"] = entry
    host_ix = host_index_with_table(api, ends)
    pinned.copy_(d_pos[:hits])
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    api.local_positions_host(host_ix, pinned.numpy().view(np.uint64), threads=args.host_threads, out_sequence=host_seq, out_local=host_local)
    t2 = time.perf_counter()
    result["host_path_protein_R570000"] = {"download_ms": result["host_path_genome_R640"]["download_ms"], "map_ms": round((t2 - t1) * 1e3, 2),
                                           "threads": args.host_threads}
    result["protein_pass_beats_host_path"] = bool(entry["median_ms"] < result["host_path_protein_R570000"]["download_ms"] + result["host_path_protein_R570000"]["map_ms"])
    host_ix.dealloc()

    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def host_index_with_table(api, ends):
    """a host index whose record table has these ends: a FASTA file of one-residue records would do for the definition but not
    for the sizes, so the table is attached to a tiny index the way the library's own reader does it -- through an .awfmi file
    whose trailer is written here (include/AwFmIndex.h; csrc/awfm_fasta.c describes the trailer)"""
    import tempfile
    tmp = tempfile.mkdtemp()
    fa = os.path.join(tmp, "one.fa")
    with open(fa, "w") as f:
        f.write(">r\nacgt\n")
    ix = api.create_index_from_fasta(fa, api.AwFmAlphabetDna, 2, 2, file_src=os.path.join(tmp, "one.awfmi"))
    ix.dealloc()
    # the trailer: header length, record count (size_t each), header characters, then {headerEndPosition, sequenceEndPosition}
    data = open(os.path.join(tmp, "one.awfmi"), "rb").read()
    tail = np.array([1, 1], np.uint64).tobytes() + b"r" + np.array([1, 4], np.uint64).tobytes()
    assert data.endswith(tail), "the .awfmi trailer is not where this script expects it"
    records = np.empty((len(ends), 2), np.uint64)
    records[:, 0] = 1
    records[:, 1] = ends
    with open(os.path.join(tmp, "big.awfmi"), "wb") as f:
        f.write(data[:-len(tail)] + np.array([1, len(ends)], np.uint64).tobytes() + b"r" + records.tobytes())
    return api.read_index_from_file(os.path.join(tmp, "big.awfmi"))


if __name__ == "__main__":
    main()
