#!/usr/bin/env python3
"""Times awfmGpuInsertHistogram + awfmGpuInsertInterval and awfmGpuPairMatesEstimated on the batch of scripts/pair_mates_timing.py
(its prepare(): 2^19 pairs x 4 slots on the 3.1 Gbp synthetic index, the slot scores written by a real awfmGpuScoreChainsAffine
call, everything resident on the device).  Device events around every one of --steps calls after --warmup, the sides taking
turns call by call in one process; spreads as min / median / max.

  new calls   the histogram zeroed (the caller's duty), awfmGpuInsertHistogram over a range of 4096 bins [0, 4095], minScore 30,
              minQuality 1, and awfmGpuInsertInterval with spread 2, minSamples 16: three enqueues, no host wait.
  (a) bar     against what a caller writes today, here in torch: the best slot per read by a keyed maximum over its scores, the
              gathers, T, the masks, bincount, cumsum and searchsorted -- no .item(), nothing comes to the host.  It yields the
              same minInsert, maxInsert and quartiles, checked equal in the same run.  Met when the comparator's median exceeds
              the new calls' by more than the sum of the two sides' max - min.
  (b)         against a device-to-device copy of the histogram call's compulsory bytes: per pair 2 C scores, one sequence, read
              end and text end per mate, three offsets and two qualities.  A ratio, not a bar.
  (c) bar     awfmGpuPairMates of this tree against the same call of --parent-lib, the library built from the parent commit,
              loaded beside this one: same image, same arrays, the calls taking turns.  Met when this tree's median exceeds the
              parent's by no more than the sum of the two spreads.  awfmGpuPairMatesEstimated (the interval read from the
              estimate the new calls wrote) beside them.  Without --parent-lib: not measured.
  (d)         every output of the new calls against the host twins over all pairs: the histogram, both counters, the eight fields
              of the estimate, and every output of the estimated pairing against awfmPairMates with the estimated interval.

Prints one JSON line and writes it to --out (default profiles/insert_size/timing.json)."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pair_mates_timing as pmt  # noqa: E402

INSERT = dict(low_template=0, high_template=4095, min_score=pmt.MIN_SCORE, min_quality=1, spread=2, min_samples=16, fallback_min=0, fallback_max=4095)
MAX_INSERT = 1 << 40


def torch_estimate(torch, slot_scores, slot_sequences, slot_read_ends, slot_text_ends, char_offsets, qualities, slots):
    """comparator (a): the histogram, the quartiles and the interval from the flat device arrays the new calls read"""
    dev, R = slot_scores.device, slot_scores.numel() // slots
    low, bins = INSERT["low_template"], INSERT["high_template"] - INSERT["low_template"] + 1
    score = (slot_scores.long() & 0xFFFFFFFF).view(R, slots)
    lengths = char_offsets[1:] - char_offsets[:-1]
    counts = (score < 0xFFFFFFFC) & (score >= max(INSERT["min_score"], 1)) & (lengths >= 0).unsqueeze(1)
    # each read's best slot: the largest score, ties to the lowest slot
    best_key = torch.where(counts, score * 16 + (15 - torch.arange(slots, device=dev)), torch.zeros_like(score)).max(1)[0]
    has = best_key > 0
    at = torch.arange(R, device=dev) * slots + torch.where(has, 15 - (best_key & 15), torch.zeros_like(best_key))
    sequence = slot_sequences[at]
    start = slot_text_ends[at] - (slot_read_ends[at].long() & 0xFFFFFFFF)
    good = has & (qualities >= INSERT["min_quality"])
    qualifies = good[0::2] & good[1::2] & (sequence[0::2] == sequence[1::2])
    T = start[1::2] + lengths[1::2] - start[0::2]
    sample = qualifies & (T >= low) & (T <= INSERT["high_template"])
    histogram = torch.bincount(torch.where(sample, T - low, torch.full_like(T, bins)), minlength=bins + 1)[:bins]
    prefix = torch.cumsum(histogram, 0)
    ranks = (torch.arange(1, 4, device=dev) * prefix[-1] + 3) // 4
    quartiles = low + torch.searchsorted(prefix, ranks)
    w = INSERT["spread"] * torch.clamp(quartiles[2] - quartiles[0], min=1)
    interval = torch.stack((torch.clamp(quartiles[0] - w, min=-MAX_INSERT), torch.clamp(quartiles[2] + w, max=MAX_INSERT)))
    return {"histogram": histogram, "quartiles": quartiles, "interval": interval}


def main():
    parser = pmt.arguments(os.path.join("profiles", "insert_size", "timing.json"))
    parser.add_argument("--parent-lib", default="", help="libawfmindex_amd.so built from the parent commit, for (c)")
    args = parser.parse_args()
    w = pmt.prepare(args)
    np, torch, api, g, dev, stream_obj, stream, timed, result = w.np, w.torch, w.api, w.g, w.dev, w.stream_obj, w.stream, w.timed, w.result
    R, P, d_char_offsets, cand, scored, SLOTS = w.R, w.P, w.d_char_offsets, w.cand, w.scored, pmt.SLOTS
    result["parameters"]["insert"] = dict(INSERT)
    bins = INSERT["high_template"] - INSERT["low_template"] + 1
    summary = pmt.summary

    def spread(s):
        return s["max_ms"] - s["min_ms"]

    # ---- the new calls ----
    pin = api.pair_inputs(d_char_offsets.data_ptr(), cand["sequences"].data_ptr(), scored["slotScores"].data_ptr(), scored["slotReadEnds"].data_ptr(),
                          scored["slotTextEnds"].data_ptr(), scored["mappingQualities"].data_ptr())
    params = api.insert_params(**INSERT)
    d_histogram = torch.zeros(bins, dtype=torch.int64, device=dev)
    d_counters = torch.zeros(2, dtype=torch.int64, device=dev)
    d_estimate = torch.zeros(8, dtype=torch.int64, device=dev)

    def new_calls():
        with torch.cuda.stream(stream_obj):
            d_histogram.zero_()
        g.insert_histogram(pin, P, params, d_histogram.data_ptr(), d_counters.data_ptr(), d_counters.data_ptr() + 8, max_candidates=SLOTS, stream=stream)
        g.insert_interval(d_histogram.data_ptr(), params, d_estimate.data_ptr(), stream=stream)

    # ---- (b) the copy of the histogram call's compulsory bytes ----
    bytes_in = P * (2 * SLOTS * 4 + 2 * (4 + 4 + 8) + 3 * 8 + 2)
    d_from, d_to = torch.zeros(bytes_in, dtype=torch.uint8, device=dev), torch.empty(bytes_in, dtype=torch.uint8, device=dev)

    def copy_call():
        with torch.cuda.stream(stream_obj):
            d_to.copy_(d_from)

    # ---- (a) the comparator ----
    old = {}

    def torch_call():
        with torch.cuda.stream(stream_obj):
            old.update(torch_estimate(torch, scored["slotScores"], cand["sequences"], scored["slotReadEnds"], scored["slotTextEnds"], d_char_offsets,
                                      scored["mappingQualities"], SLOTS))

    ours, copies, theirs = (summary(ms) for ms in timed(new_calls, copy_call, torch_call))
    calls = args.steps + args.warmup

    # ---- (c) the pairing call of this tree, of the parent's build, and the estimated one ----
    new_out = {name: torch.zeros(P * per, dtype=getattr(torch, dtype), device=dev) for name, dtype, per in pmt.PAIR_FIELDS}
    d_pair_counters = torch.zeros(2, dtype=torch.int64, device=dev)
    pout = api.pair_outputs(numProper=d_pair_counters.data_ptr(), numWindows=d_pair_counters.data_ptr() + 8,
                            **{name: t.data_ptr() for name, t in new_out.items()})
    settings = dict(max_candidates=SLOTS, min_score=pmt.MIN_SCORE, unpaired_penalty=pmt.UNPAIRED_PENALTY, window_pad=pmt.WINDOW_PAD, mapq_cap=pmt.MAPQ_CAP)
    pair_params = api.pair_params(pmt.MIN_INSERT, pmt.MAX_INSERT, pmt.MIN_SCORE, pmt.UNPAIRED_PENALTY, pmt.WINDOW_PAD, pmt.MAPQ_CAP)

    def pairing_call():
        g.pair_mates(pin, P, pout, pmt.MIN_INSERT, pmt.MAX_INSERT, stream=stream, **settings)

    def estimated_call():
        g.pair_mates_estimated(pin, P, pout, d_estimate.data_ptr(), stream=stream, **settings)

    sides = [pairing_call, estimated_call]
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        parent.awfmGpuPairMates.restype = C.c_int
        parent.awfmGpuPairMates.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]

        def parent_call():
            assert parent.awfmGpuPairMates(g.handle, C.byref(pin), P, SLOTS, C.byref(pair_params), C.byref(pout), stream) == 1

        sides.append(parent_call)
    pairing_ms = [summary(ms) for ms in timed(*sides)]
    estimated_call()  # once more: whichever side wrote last, (d) compares the estimated call's outputs
    stream_obj.synchronize()

    # ---- (d) the host twins on the same arrays, all pairs ----
    host_offsets = d_char_offsets.cpu().numpy().astype(np.uint64)
    host_slots = {"sequences": cand["sequences"], "slotScores": scored["slotScores"], "slotReadEnds": scored["slotReadEnds"],
                  "slotTextEnds": scored["slotTextEnds"]}
    host_slots = {name: t.cpu().numpy().view(dtype).reshape(R, SLOTS) for (name, t), dtype in zip(host_slots.items(), (np.uint32, np.uint32, np.uint32, np.uint64))}
    host_qualities = scored["mappingQualities"].cpu().numpy()
    want = api.estimate_insert_size_host(host_offsets, host_slots, params, mapping_qualities=host_qualities, threads=args.threads)
    got = api.insert_estimate_dict(d_estimate.cpu().numpy())
    counters = d_counters.cpu().numpy()
    equal = {"histogram": bool(np.array_equal(d_histogram.cpu().numpy().view(np.uint64), want["histogram"])),
             "numSamples": int(counters[0]) == calls * want["numSamples"], "numOutside": int(counters[1]) == calls * want["numOutside"],
             "estimate": all(got[name] == want[name] for name in api.INSERT_ESTIMATE_FIELDS)}
    paired = api.pair_mates_host(host_offsets, host_slots, want["minInsert"], want["maxInsert"], mapping_qualities=host_qualities, min_score=pmt.MIN_SCORE,
                                 unpaired_penalty=pmt.UNPAIRED_PENALTY, window_pad=pmt.WINDOW_PAD, mapq_cap=pmt.MAPQ_CAP, threads=args.threads)
    pairing_equal = {name: bool(np.array_equal(new_out[name].cpu().numpy().view(paired[name].dtype), paired[name])) for name, _, _ in pmt.PAIR_FIELDS}
    comparator_equal = {"histogram": bool(torch.equal(old["histogram"], d_histogram)),
                        "quartiles": [int(v) for v in old["quartiles"].cpu()] == want["quartiles"],
                        "interval": [int(v) for v in old["interval"].cpu()] == [want["minInsert"], want["maxInsert"]]}

    result.update(new_calls=ours, copy_of_compulsory_bytes=copies, torch_comparator=theirs, compulsory_bytes=bytes_in, bins=bins,
                  estimate={name: want[name] for name in api.INSERT_ESTIMATE_FIELDS}, samples=want["numSamples"], outside=want["numOutside"],
                  pairs_compared=P, results_equal=all(equal.values()), results_equal_by_output=equal,
                  estimated_pairing_equal=all(pairing_equal.values()), estimated_pairing_equal_by_output=pairing_equal,
                  estimated_pairing_proper_pairs=paired["numProper"], torch_comparator_equal=all(comparator_equal.values()),
                  torch_comparator_equal_by_output=comparator_equal, new_calls_over_copy=round(ours["median_ms"] / copies["median_ms"], 3),
                  bar_a={"summed_spreads_ms": round(spread(ours) + spread(theirs), 4), "speedup": round(theirs["median_ms"] / ours["median_ms"], 3),
                         "met": bool(theirs["median_ms"] - ours["median_ms"] > spread(ours) + spread(theirs))},
                  pair_mates_this_tree=pairing_ms[0], pair_mates_estimated=pairing_ms[1])
    if args.parent_lib:
        slower = pairing_ms[0]["median_ms"] - pairing_ms[2]["median_ms"]
        result.update(pair_mates_parent=pairing_ms[2],
                      bar_c={"summed_spreads_ms": round(spread(pairing_ms[0]) + spread(pairing_ms[2]), 4), "this_tree_minus_parent_ms": round(slower, 4),
                             "met": bool(slower <= spread(pairing_ms[0]) + spread(pairing_ms[2]))})
    else:
        result["bar_c"] = "not measured: no --parent-lib"

    text = json.dumps(result)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
