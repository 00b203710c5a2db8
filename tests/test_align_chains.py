"""awfmAlignChains (include/awfm_gpu.h "chain alignment", csrc/awfm_align.c), the host twin and checker of awfmGpuAlignChains:
against a plain-Python restatement of the definition (dict of cells, exact integers, the direction and end rules as written) on
random batches, against an unbanded fitting dynamic programme (never smaller; equal on planted reads), by replaying every edit
script over read and text, on the edge list with hand-computed values, and as a stand-alone program under AddressSanitizer and
UBSan."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_chains_common as ac  # noqa: E402
import verify_chains_common as vc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "avxwindowfmindex_amd", "csrc")
ALL_OUTPUTS = list(ac.READ_OUTPUTS) + ["ops"] + list(ac.COUNTERS)


def assert_scripts_replay(case, got, w, x, max_ops):
    """for every aligned, untruncated read: the runs cover the read and T[textBegin, textEnd), split '=' from X as the letters
    say, and hold as many X, I and D characters as the distance"""
    replayed = 0
    for r in range(case.num_reads):
        status = case.status(r, w, x)
        k = int(got["numOps"][r])
        if not isinstance(status, tuple) or k > max_ops:
            continue
        S = status[0]
        begin, end = int(got["textBegins"][r]), int(got["textEnds"][r])
        R, T = case.read(r), bytes(case.text[S + begin:S + end])
        assert ac.replay(ac.runs_of(got["ops"][r], k), R, T, case.alphabet) == (len(R), len(T), int(got["editDistances"][r])), r
        assert status[2] <= begin <= end <= status[1] - S  # inside the record, not before the band's first diagonal
        replayed += 1
    return replayed


@pytest.mark.parametrize("alphabet,C,w,x", [(ac.DNA, 4, 0, 0), (ac.AMINO, 1, 7, 0), (ac.DNA, 16, 7, 1), (ac.AMINO, 4, 8, 0), (ac.DNA, 1, 15, 0),
                                            (ac.DNA, 4, 15, 1), (ac.AMINO, 16, 16, 0), (ac.DNA, 4, 31, 0), (ac.AMINO, 1, 31, 1), (ac.DNA, 4, 2, 3)])
def test_random_batches_equal_the_python_restatement_and_replay(awfm, alphabet, C, w, x):
    """band widths 1, 15, 16, 17, 31, 32, 33, 63, 64 and 8; some slots unused, some malformed, some overhanging"""
    case = ac.random_case(13 * C + w + x, 60 if C < 16 else 40, C, alphabet, max_length=40 + 2 * w, broken=0.08, hanging=0.3)
    max_ops = 12
    want = case.expected(w, x, max_ops, unaligned_before=5, truncated_before=7)
    got = case.host(awfm, w, x, max_ops, unaligned_before=5, truncated_before=7, fill=0x5A, threads=3)
    ac.assert_equal(got, want, what=f"C={C} w={w} x={x}", fill=0x5A)
    kinds = set(int(v) for v in want["editDistances"] if v >= ac.OVERHANG)
    assert {ac.NONE, ac.MALFORMED, ac.OVERHANG} <= kinds and want["numUnaligned"] > 5
    assert assert_scripts_replay(case, got, w, x, max_ops) >= 5  # (with x = 0 every read with an indel in its chain is too wide)
    for r in range(case.num_reads):  # an upper bound of the unbanded fitting distance of the read against the record
        status = case.status(r, w, x)
        if isinstance(status, tuple):
            assert int(got["editDistances"][r]) >= ac.unbanded_fitting(case.read(r), bytes(case.text[status[0]:status[1]]), alphabet), r


def test_a_band_of_65_diagonals_and_other_arguments_out_of_range_are_refused(awfm):
    case = ac.edge_builder(2, 3).case()
    for kw in (dict(w=32, x=0), dict(w=0, x=64), dict(w=31, x=2), dict(w=2 ** 31, x=2 ** 31), dict(w=2, x=3, max_ops=0),
               dict(w=2, x=3, max_ops=ac.MAX_OPS + 1)):
        with pytest.raises(awfm.AwFmError) as e:
            case.host(awfm, **kw)
        assert e.value.rc == awfm.AwFmIllegalPositionError, kw
    assert case.host(awfm, 0, 63, max_ops=ac.MAX_OPS)["ops"].shape == (case.num_reads, ac.MAX_OPS)
    lib = awfm._lib.lib()
    empty = awfm.verify_inputs(0, 0, 0)
    assert lib.awfmAlignChains(empty, None, 0, 4, 2, 3, 8, None, 0, None, 0, ac.DNA, None, 1) == awfm.AwFmSuccess  # no reads: nothing touched
    assert lib.awfmAlignChains(empty, None, 1, 4, 2, 3, 8, None, 0, None, 0, ac.DNA, awfm.align_outputs(), 1) == -4  # AwFmNullPtrError
    slots = {name: np.zeros((1, 1), vc.SLOT_DTYPES[name]) for name in vc.SLOT_FIELDS}
    vin = awfm.verify_inputs(case.read_chars.ctypes.data, 4, case.offsets.ctypes.data, **{n: a.ctypes.data for n, a in slots.items()})
    assert lib.awfmAlignChains(vin, None, 1, 1, 2, 3, 8, case.text.ctypes.data, case.text.size, None, 0, ac.DNA, awfm.align_outputs(), 1) == -4
    for C in (0, 17):
        rc = lib.awfmAlignChains(vin, case.chosen.ctypes.data, 1, C, 2, 3, 8, case.text.ctypes.data, case.text.size, None, 0, ac.DNA,
                                 awfm.align_outputs(), 1)
        assert rc == awfm.AwFmIllegalPositionError


def test_planted_reads_equal_the_unbanded_fitting_distance(awfm):
    """300 reads of 30..150 characters with 3 % substitutions, 1.5 % deletions and 1.5 % insertions on their true begin and end
    diagonals, w = 8: none refused, none truncated at 64 runs, every distance the unbanded one"""
    case, intervals = ac.planted_case()
    got = case.host(awfm, 8, 15, max_ops=64, threads=4)
    assert got["numUnaligned"] == 0 and got["numTruncated"] == 0 and int(got["numOps"].max()) <= 64
    equal = 0
    for r, (s, tb, te) in enumerate(intervals):
        S, E = case.record(s)
        full = ac.unbanded_fitting(case.read(r), bytes(case.text[S:E]))
        assert int(got["editDistances"][r]) >= full, r
        equal += int(got["editDistances"][r]) == full
    assert equal == case.num_reads
    assert assert_scripts_replay(case, got, 8, 15, 64) == case.num_reads


@pytest.mark.parametrize("w,x", [(2, 3), (8, 15), (3, 4), (24, 15)])
def test_edge_list_by_hand_computed_values(awfm, w, x):
    b = ac.edge_builder(w, x)
    case = b.case()
    got = case.host(awfm, w, x, max_ops=8, unaligned_before=9, truncated_before=2, fill=0xC3)
    b.check(got, 8)
    assert got["numUnaligned"] == 9 + b.unaligned() and got["numTruncated"] == 2
    ac.assert_equal(got, case.expected(w, x, 8, unaligned_before=9, truncated_before=2), what="restatement", fill=0xC3)
    assert_scripts_replay(case, got, w, x, 8)
    for skew in (1, 2, 3):  # the same reads further into their buffer
        ac.assert_equal(b.case(skew).host(awfm, w, x, max_ops=8, unaligned_before=9, truncated_before=2), got, what=f"skew {skew}")


def test_max_ops_exactly_the_number_of_runs_and_one_less(awfm):
    """guard words around every row: a row is written up to its runs or, truncated, nowhere outside itself"""
    b = ac.edge_builder(2, 3)
    case = b.case()
    full = case.host(awfm, 2, 3, max_ops=8)
    most = int(full["numOps"].max())
    assert most == 3 and full["numTruncated"] == 0
    for max_ops in (most, most - 1):
        n = case.num_reads
        # the rows of ops as the middle third of rows three times as wide: the words on either side of a row are its guards
        wide = np.full((n, 3 * max_ops), 0xA5A5A5A5, np.uint32)
        rows = {name: np.full(n + 2, 0xA5, dtype) for name, dtype in ac.READ_OUTPUTS.items()}
        counters = np.array([0xA5A5, 4, 6, 0xA5A5], np.uint64)
        lib = awfm._lib.lib()
        for r in range(n):  # a read at a time, so that every row lies between words of its own
            one = ac.Case(case.read(r), [0, len(case.read(r))], {name: case.slots[name][r:r + 1] for name in vc.SLOT_FIELDS}, case.chosen[r:r + 1],
                          case.text.tobytes(), case.ends)
            vin = awfm.verify_inputs(one.read_chars.ctypes.data if one.read_chars.size else counters.ctypes.data, one.num_read_chars,
                                     one.offsets.ctypes.data, **{name: a.ctypes.data for name, a in one.slots.items()})
            out = awfm.align_outputs(ops=wide[r, max_ops:].ctypes.data, numUnaligned=counters[1:].ctypes.data, numTruncated=counters[2:].ctypes.data,
                                     **{name: a[r + 1:].ctypes.data for name, a in rows.items()})
            assert lib.awfmAlignChains(vin, one.chosen.ctypes.data, 1, 1, 2, 3, max_ops, one.text.ctypes.data, one.text.size, one.ends.ctypes.data,
                                       len(one.ends), ac.DNA, out, 1) == awfm.AwFmSuccess
        assert (wide[:, :max_ops] == 0xA5A5A5A5).all() and (wide[:, 2 * max_ops:] == 0xA5A5A5A5).all()
        truncated = full["numOps"] > max_ops
        assert counters.tolist() == [0xA5A5, 4 + full["numUnaligned"], 6 + int(truncated.sum()), 0xA5A5] and truncated.sum() == (max_ops < most) * (full["numOps"] == most).sum()
        for name, a in rows.items():
            assert np.array_equal(a[1:-1], full[name]) and a[0] == a[-1] == 0xA5, name
        for r in range(n):
            k = int(full["numOps"][r])
            if k <= max_ops:
                assert np.array_equal(wide[r, max_ops:max_ops + k], full["ops"][r, :k]) and (wide[r, max_ops + k:2 * max_ops] == 0xA5A5A5A5).all(), r


def test_every_output_null_in_turn_and_both_counters_are_added_to(awfm):
    case = ac.random_case(3, 50, 4, hanging=0.2)
    want = case.host(awfm, 2, 3, max_ops=4)
    assert want["numUnaligned"] > 0 and want["numTruncated"] > 0
    for missing in ALL_OUTPUTS:
        for outputs in ([n for n in ALL_OUTPUTS if n != missing], [missing]):
            got = case.host(awfm, 2, 3, max_ops=4, outputs=outputs, fill=0xC3)
            assert sorted(got) == sorted(outputs)
            ac.assert_equal(got, want, names=outputs, what=str(outputs))
    got = case.host(awfm, 2, 3, max_ops=4, unaligned_before=2 ** 40, truncated_before=2 ** 41)
    assert got["numUnaligned"] == 2 ** 40 + want["numUnaligned"] and got["numTruncated"] == 2 ** 41 + want["numTruncated"]


def test_read_offsets_that_are_inverted_or_leave_the_buffer(awfm):
    b = ac.Builder([b"gatcctgaagtcatgc"])
    for k in range(4):
        b.add(f"read {k}", b"gatcctgaagtcatgc"[4 * k:4 * k + 4], 0, 4 * k, 4 * k, None)
    case = b.case()
    case.offsets = np.array([0, 4, 3, 12, 17], np.uint64)  # read 1 inverted, read 2 nine characters long, read 3 beyond the 16
    got = case.host(awfm, 2, 3)
    assert got["editDistances"].tolist() == [0, ac.MALFORMED, int(case.expected(2, 3)["editDistances"][2]), ac.MALFORMED]
    assert got["numUnaligned"] == 2
    ac.assert_equal(got, case.expected(2, 3))
    case.num_read_chars = 11  # now read 2 leaves it too
    assert case.host(awfm, 2, 3)["editDistances"].tolist() == [0, ac.MALFORMED, ac.MALFORMED, ac.MALFORMED]


@pytest.mark.parametrize("length", range(96, 112))
def test_last_record_ending_at_the_texts_last_byte(awfm, length):
    b = ac.tail_case(length)
    got = b.case().host(awfm, 2, 3)
    b.check(got, 32)


def test_one_sequence_without_a_record_table_and_the_amino_alphabet(awfm):
    slots = {name: np.array([[v]], vc.SLOT_DTYPES[name]) for name, v in zip(vc.SLOT_FIELDS, (0, 1, 0, 4, 2, 2))}
    got = ac.Case(b"ARXD", [0, 4], slots, [0], b"mkarxdmk", None, ac.AMINO).host(awfm, 1, 1)
    # x matches nothing, not even itself; case is ignored
    assert (int(got["editDistances"][0]), int(got["textBegins"][0]), int(got["textEnds"][0]), ac.cigar(ac.runs_of(got["ops"][0], 3))) == (1, 2, 6, "2=1X1=")
    slots["sequences"][0, 0] = 1
    assert int(ac.Case(b"ARXD", [0, 4], slots, [0], b"mkarxdmk", None, ac.AMINO).host(awfm, 1, 1)["editDistances"][0]) == ac.MALFORMED
    slots["sequences"][0, 0] = 0
    got = ac.Case(b"ARND", [0, 4], slots, [0], b"mkarndmk", None, ac.AMINO).host(awfm, 1, 1)
    assert (int(got["editDistances"][0]), ac.cigar(ac.runs_of(got["ops"][0], int(got["numOps"][0])))) == (0, "4=")
    got = ac.Case(b"acgt", [0, 4], slots, [0], b"ttACGTtt", None, ac.DNA).host(awfm, 0, 0)
    assert (int(got["editDistances"][0]), int(got["textBegins"][0]), int(got["textEnds"][0])) == (0, 2, 6)


def long_case(n=ac.MAX_LENGTH):
    """a record of n + 40 characters and two reads on diagonal 20: one of n characters with five substitutions, one of n + 1"""
    rng = np.random.default_rng(20)
    text = rng.choice(np.frombuffer(b"acgt", np.uint8), n + 40)
    read = text[20:20 + n + 1].copy()
    for at in (0, 1000, n // 2, n - 2, n - 1):
        read[at] = ord("n")
    slots = {name: np.array([[0], [0]], vc.SLOT_DTYPES[name]) for name in vc.SLOT_FIELDS}
    slots["chainAnchors"][:] = 1
    slots["chainReadEnds"][:, 0] = (n, n + 1)
    slots["chainBeginDiagonals"][:] = slots["chainEndDiagonals"][:] = 20
    return ac.Case(read[:n].tobytes() + read.tobytes(), [0, n, 2 * n + 1], slots, [0, 0], text.tobytes() + b"\0", [n + 40])


def test_too_long_at_two_to_the_sixteen_and_one_more(awfm):
    n = ac.MAX_LENGTH
    got = long_case().host(awfm, 8, 15)
    assert got["editDistances"].tolist() == [5, ac.TOO_LONG] and got["numUnaligned"] == 1 and got["numTruncated"] == 0
    # the first and the last character are substituted: the first stays an X (the diagonal counts), the last two become
    # (as two I: of the ends at distance 5 the leftmost counts)
    assert (int(got["textBegins"][0]), int(got["textEnds"][0])) == (20, 20 + n - 2)
    assert ac.cigar(ac.runs_of(got["ops"][0], int(got["numOps"][0]))) == f"1X999=1X{n // 2 - 1001}=1X{n - 3 - n // 2}=2I"


def assert_planted_reads_aligned(case, got, planted, band_pad, read_length=120):
    """end to end: every planted read's locus lies at least band_pad inside its record, the read is aligned to its record at a
    distance of at most the edits planted in the whole read, [textBegin, textEnd) lies within band_pad of the planted interval,
    and the edit script replays"""
    for r, plant in enumerate(planted):
        if plant is None:
            continue
        record, at, deleted = plant
        S, E = case.record(record)
        end = at + read_length + (1 if deleted else 0)
        assert at >= band_pad and end + band_pad <= E - S, (r, plant)
        j = int(case.chosen[r])
        assert j != ac.NO_SLOT and case.slots["sequences"][r, j] == record, (r, plant)
        distance = int(got["editDistances"][r])
        assert distance <= 4 + (1 if deleted else 0), (r, plant, distance)
        begin, stop, k = int(got["textBegins"][r]), int(got["textEnds"][r]), int(got["numOps"][r])
        assert abs(begin - at) <= band_pad and abs(stop - end) <= band_pad, (r, plant, begin, stop)
        assert k <= got["ops"].shape[1]
        R, T = case.read(r), bytes(case.text[S + begin:S + stop])
        assert ac.replay(ac.runs_of(got["ops"][r], k), R, T) == (len(R), len(T), distance), (r, plant)


def test_end_to_end_on_the_host_aligns_every_planted_read(awfm, tmp_path):
    """FASTA -> longest matches -> located -> mapped -> candidates -> chains -> verification -> alignment, all host twins"""
    import read_candidates_common as rc
    import read_chains_common as ch
    fa, records, reads, planted = ac.planted_inside(str(tmp_path), vc.E2E_W)
    ix = awfm.create_index_from_fasta(fa, awfm.AwFmAlphabetDna, 8, 8, file_src=str(tmp_path / "records.awfmi"))
    try:
        host = rc.host_pipeline(awfm, ix, reads)
    finally:
        ix.dealloc()
    chain_case = ch.candidate_case(awfm, host, 2, 4, max_hits_per_seed=rc.E2E_MAX_HITS, min_votes=2)
    chains = chain_case.host(awfm, max_hits_per_seed=rc.E2E_MAX_HITS, band=2, gap_penalty=1)
    text, ends = vc.text_of(records)
    slots = dict({name: chains[name] for name in vc.SLOT_FIELDS[1:]}, sequences=chain_case.sequences)
    offsets = np.arange(len(reads) + 1) * rc.E2E_READ_LENGTH
    verified = vc.Case(b"".join(reads), offsets, slots, text.tobytes(), ends).host(awfm, vc.E2E_W, vc.E2E_X)
    case = ac.Case(b"".join(reads), offsets, slots, verified["bestSlots"], text.tobytes(), ends)
    got = case.host(awfm, vc.E2E_W, vc.E2E_X, max_ops=32)
    assert got["numTruncated"] == 0
    assert_planted_reads_aligned(case, got, planted, vc.E2E_W)


SANITIZER_MAIN = r"""
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "awfm_gpu.h"
static void *block(FILE *f, size_t bytes) { /* a heap block of exactly its size: the sanitizer sees every read outside it */
  void *p = malloc(bytes ? bytes : 1);
  if (bytes && fread(p, 1, bytes, f) != bytes) exit(2);
  return p;
}
int main(int argc, char **argv) {
  FILE *f = argc < 2 ? NULL : fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t h[12];
  if (fread(h, 8, 12, f) != 12) return 2;
  const uint64_t numReads = h[0], slots = h[1], sizeChars = h[2], textLength = h[4], numRecords = h[5], n = numReads * slots, maxOps = h[11];
  struct AwFmVerifyInputs in = {0};
  in.numReadChars = h[3];
  in.readChars = block(f, sizeChars);
  in.readOffsets = block(f, (numReads + 1) * 8);
  in.sequences = block(f, n * 4);
  in.chainAnchors = block(f, n * 4);
  in.chainReadBegins = block(f, n * 4);
  in.chainReadEnds = block(f, n * 4);
  in.chainBeginDiagonals = block(f, n * 8);
  in.chainEndDiagonals = block(f, n * 8);
  const uint32_t *chosen = block(f, numReads * 4);
  const uint8_t *text = block(f, textLength);
  const uint64_t *ends = numRecords ? block(f, numRecords * 8) : NULL;
  uint64_t unaligned = h[9], truncated = h[9] + 1;
  struct AwFmAlignOutputs out = {malloc(numReads * 4), malloc(numReads * 8), malloc(numReads * 8), malloc(numReads * 4),
                                 calloc(numReads * maxOps, 4), &unaligned, &truncated};
  if (awfmAlignChains(&in, chosen, numReads, (uint32_t)slots, (uint32_t)h[6], (uint32_t)h[7], (uint32_t)maxOps, text, textLength, ends,
                      numRecords, (int)h[8], &out, (unsigned)h[10]) != AwFmSuccess)
    return 3;
  fwrite(out.editDistances, 4, numReads, stdout);
  fwrite(out.textBegins, 8, numReads, stdout);
  fwrite(out.textEnds, 8, numReads, stdout);
  fwrite(out.numOps, 4, numReads, stdout);
  fwrite(out.ops, 4, numReads * maxOps, stdout);
  fwrite(&unaligned, 8, 1, stdout);
  fwrite(&truncated, 8, 1, stdout);
  return 0;
}
"""


def test_host_twin_under_address_and_undefined_sanitizers(awfm, tmp_path):
    """the twin indexes the read buffer, the text and its direction table by offsets and diagonals its caller supplies:
    awfm_align.c, the letter tables and the thread pool, compiled with a stand-alone main under -fsanitize=address,undefined, run
    on the edge list (every malformed shape in it), on the tails that end at the text's last byte and on random batches spread
    over four threads, every array in a heap block of exactly its size"""
    (tmp_path / "main.c").write_text(SANITIZER_MAIN)
    exe = str(tmp_path / "align_asan")
    subprocess.check_call(["gcc", "-std=gnu11", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-pthread", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, str(tmp_path / "main.c"),
                           os.path.join(CSRC, "awfm_align.c"), os.path.join(CSRC, "awfm_letters.c"), os.path.join(CSRC, "awfm_threads.c"),
                           "-o", exe])
    cases = [("edge", ac.edge_builder(2, 3).case(), 2, 3, 2, 2), ("edge-wide", ac.edge_builder(24, 15).case(3), 24, 15, 1, 8),
             ("tail", ac.tail_case(113).case(), 2, 3, 1, 4), ("random", ac.random_case(8, 400, 4, max_length=80, hanging=0.2), 4, 7, 4, 6),
             ("amino", ac.random_case(9, 100, 16, ac.AMINO, hanging=0.2), 8, 15, 4, 64)]
    for name, case, w, x, threads, max_ops in cases:
        header = np.array([case.num_reads, case.C, case.read_chars.size, case.num_read_chars, case.text.size, len(case.ends), w, x, case.alphabet,
                           6, threads, max_ops], np.uint64)
        arrays = [header, case.read_chars, case.offsets] + [case.slots[f] for f in vc.SLOT_FIELDS] + [case.chosen, case.text, case.ends]
        (tmp_path / name).write_bytes(b"".join(a.tobytes() for a in arrays))
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
        run = subprocess.run([exe, str(tmp_path / name)], capture_output=True, env=env, timeout=120)
        assert run.returncode == 0, (name, run.stderr.decode(errors="replace")[-3000:])
        want = case.host(awfm, w, x, max_ops, unaligned_before=6, truncated_before=7)
        n, at, got = case.num_reads, 0, {}
        for field, dtype, count in (("editDistances", np.uint32, n), ("textBegins", np.uint64, n), ("textEnds", np.uint64, n),
                                    ("numOps", np.uint32, n), ("ops", np.uint32, n * max_ops), ("numUnaligned", np.uint64, 1),
                                    ("numTruncated", np.uint64, 1)):
            got[field] = np.frombuffer(run.stdout, dtype, count, at)
            at += count * np.dtype(dtype).itemsize
        got["ops"] = got["ops"].reshape(n, max_ops)
        got["numUnaligned"], got["numTruncated"] = int(got["numUnaligned"][0]), int(got["numTruncated"][0])
        ac.assert_equal(got, want, what=name)
