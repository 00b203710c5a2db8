"""The second table window of lookupSearchKernel on the headline batch (bench.py's default: 3.1 Gbp uniform text, 10^8 random
21-mers, the list form): what awfmGpuLastSecondWindow reports beside awfmGpuLastOrderedKept, and the search's time with the window
left to its gate, forced on and forced off ($AWFM_GPU_DIAG second_window) -- the three interleaved in one process, on one image.
One JSON line.  usage: python scripts/second_window_counters.py [--text-len N] [--queries Q] [--rounds R] [--workload random|planted]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--text-len", type=float, default=3.1e9)
    p.add_argument("--queries", type=float, default=1e8)
    p.add_argument("--kmer", type=int, default=21)
    p.add_argument("--rounds", type=int, default=5, help="timed rounds; a round is 4 searches per setting")
    p.add_argument("--workload", choices=["random", "planted"], default="random")
    args = p.parse_args()
    import torch
    from avxwindowfmindex_amd import _lib, api
    L = _lib.lib()
    n, Q, K = int(args.text_len), int(args.queries), args.kmer
    dev = torch.device("cuda", 0)
    d_text = torch.empty(n, dtype=torch.uint8, device=dev)
    assert L.awfmGpuSynthText(d_text.data_ptr(), 0, n, 2, 0, None) == 1
    torch.cuda.synchronize()
    ix = api.gpu_create_index(d_text.data_ptr(), api.AwFmAlphabetDna, 8, 12, on_device_length=n, device=0)
    g = api.GpuIndex(ix, acquire=True)
    d_chars = torch.empty(Q * K, dtype=torch.uint8, device=dev)
    if args.workload == "random":
        assert L.awfmGpuSynthRandomQueries(d_chars.data_ptr(), 0, Q, K, 102, 0, None) == 1
    else:
        os.environ["AWFM_GPU_LOOKUP_FIRST"] = "1"  # an all-hits batch through the lookup kernel
        assert L.awfmGpuSynthPlantedQueries(d_chars.data_ptr(), 0, Q, K, 103, d_text.data_ptr(), n, None) == 1
    del d_text
    cap = Q
    d_kmers = torch.zeros(cap, dtype=torch.int32, device=dev)
    d_ranges = torch.zeros(cap * 2, dtype=torch.int64, device=dev)
    d_num = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def search():
        g.search_hits_compact(d_chars.data_ptr(), 0, K, Q, d_kmers.data_ptr(), d_ranges.data_ptr(), cap, d_num.data_ptr())

    def setting(value):
        keys = [kv for kv in os.environ.get("AWFM_GPU_DIAG", "").split(",") if kv and not kv.startswith("second_window=")]
        if value is not None:
            keys.append(f"second_window={value}")
        os.environ["AWFM_GPU_DIAG"] = ",".join(keys)

    settings = (("gate", None), ("on", "1"), ("off", "0"))
    out = {"text_len": n, "queries": Q, "kmer": K, "workload": args.workload, "image": g.describe()}
    for _ in range(6):  # the front-end prediction settles
        search()
    torch.cuda.synchronize()
    hits = {}
    for name, value in settings:
        setting(value)
        search()
        torch.cuda.synchronize()
        tested, dropped = g.last_second_window()
        out[name] = {"lookup_kernel": g.last_ordered_kernel_is_lookup(), "kept": g.last_ordered_kept(), "tested": tested,
                     "dropped": dropped, "hits": int(d_num.item()), "ms": []}
        hits[name] = (int(d_num.item()), int(d_kmers[:int(d_num.item())].to(torch.int64).sum().item()))
    assert len(set(hits.values())) == 1, hits  # the same k-mers with hits under every setting
    for _ in range(args.rounds):
        for name, value in settings:
            setting(value)
            search()
            begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            begin.record()
            for _ in range(4):
                search()
            end.record()
            torch.cuda.synchronize()
            out[name]["ms"].append(round(begin.elapsed_time(end) / 4, 4))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
