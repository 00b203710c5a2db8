"""awfmVerifyChains (include/awfm_gpu.h "chain verification", csrc/awfm_verify.c), the host twin and checker of
awfmGpuVerifyChains: against a plain-Python restatement of the definition (dict of cells, exact integers, the band rule as
written) on random batches, against an unbanded full dynamic programme (equal wherever the full distance is <= 2 w + |delta|,
never smaller), on the edge list with hand-computed values, and as a stand-alone program under AddressSanitizer and UBSan."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import verify_chains_common as vc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "avxwindowfmindex_amd", "csrc")


@pytest.mark.parametrize("alphabet,C,w,x", [(vc.DNA, 4, 2, 3), (vc.AMINO, 1, 3, 5), (vc.DNA, 16, 0, 4), (vc.AMINO, 3, 8, 15), (vc.DNA, 2, 1, 0)])
def test_random_batches_equal_the_python_restatement_and_bound_the_full_distance(awfm, alphabet, C, w, x):
    case = vc.random_case(11 * C + w, 80 if C < 16 else 30, C, alphabet, max_length=40, broken=0.08)
    want = case.expected(w, x, unverified_before=5)
    got = case.host(awfm, w, x, unverified_before=5, fill=0x5A, threads=3)
    vc.assert_equal(got, want, what=f"C={C} w={w} x={x}")
    kinds = set(int(v) for v in want["editDistances"].reshape(-1) if v >= vc.TOO_LONG)
    assert {vc.NONE, vc.MALFORMED} <= kinds and want["numUnverified"] > 5
    exact = 0
    for r in range(case.num_reads):
        for j in range(C):
            d = int(want["editDistances"][r, j])
            if d >= vc.TOO_LONG:
                continue
            R, T = case.intervals(r, j)
            full = vc.unbanded(R, T, alphabet)
            assert d >= full, (r, j, d, full)
            if full <= 2 * w + abs(len(T) - len(R)):
                assert d == full, (r, j, d, full)
                exact += 1
    assert exact > case.num_reads // 4  # (most planted slots; with x = 0 every indel makes a slot too wide)


@pytest.mark.parametrize("w,x", [(2, 3), (8, 15), (3, 4), (24, 15)])
def test_edge_list_by_hand_computed_values(awfm, w, x):
    b = vc.edge_builder(w, x)
    case = b.case()
    got = case.host(awfm, w, x, unverified_before=9)
    bad = [(name, int(g), int(v)) for name, g, v in zip(b.names, got["editDistances"][:, 0], b.values) if g != v]
    assert not bad, bad
    unverified = sum(v in (vc.MALFORMED, vc.TOO_WIDE, vc.TOO_LONG) for v in b.values)
    assert got["numUnverified"] == 9 + unverified
    assert np.array_equal(got["bestSlots"], np.where(b.want()[:, 0] >= vc.TOO_LONG, vc.NO_SLOT, 0))
    vc.assert_equal(got, case.expected(w, x, unverified_before=9), what="restatement")
    for skew in (1, 2, 3):  # the same reads further into their buffer
        vc.assert_equal(b.case(skew).host(awfm, w, x, unverified_before=9), got, what=f"skew {skew}")


def test_indel_run_of_w_and_of_w_plus_one(awfm):
    """the read deletes "tt" and inserts it ten characters later: 4 inside a band of +-2 (the unbanded distance), more than 4
    inside +-1, where the path cannot reach the diagonal it needs; pure Hamming at w = 0"""
    read, text = b"acgtacgtacttgcagcagcag", b"acgtacgtacgcagcagcagtt"
    assert vc.unbanded(read, text) == 4 and vc.banded(read, text, 2) == 4
    narrow, hamming = vc.banded(read, text, 1), sum(p != q for p, q in zip(read, text))
    assert 4 < narrow <= hamming == vc.banded(read, text, 0) == 12
    for w, value in ((2, 4), (1, narrow), (0, hamming)):
        b = vc.Builder([text])
        b.add("run", read, 0, 22, 0, 0, 22, value)
        assert int(b.case().host(awfm, w, 0)["editDistances"][0, 0]) == value, w


@pytest.mark.parametrize("width", sorted(vc.BAND_SHAPES))
def test_band_widths(awfm, width):
    w, x = vc.BAND_SHAPES[width]
    assert x + 2 * w + 1 == width
    b = vc.band_shape_case(w, x)
    case = b.case()
    R, T = case.intervals(0, 0)
    assert vc.unbanded(R, T) == 2
    got = case.host(awfm, w, x)
    assert np.array_equal(got["editDistances"], b.want()), (got["editDistances"].tolist(), b.values)
    vc.assert_equal(got, case.expected(w, x))


def test_a_band_of_65_diagonals_is_refused_and_errors_follow_the_chain_call(awfm):
    case = vc.edge_builder(2, 3).case()
    for w, x in ((32, 0), (0, 64), (31, 2), (2 ** 31, 2 ** 31)):
        with pytest.raises(awfm.AwFmError) as e:
            case.host(awfm, w, x)
        assert e.value.rc == awfm.AwFmIllegalPositionError
    assert case.host(awfm, 0, 63)["editDistances"].shape == (case.num_reads, 1)
    lib = awfm._lib.lib()
    empty = awfm.verify_inputs(0, 0, 0)
    assert lib.awfmVerifyChains(empty, 0, 4, 2, 3, None, 0, None, 0, vc.DNA, None, 1) == awfm.AwFmSuccess  # no reads: nothing touched
    assert lib.awfmVerifyChains(empty, 1, 4, 2, 3, None, 0, None, 0, vc.DNA, awfm.verify_outputs(), 1) == -4  # AwFmNullPtrError
    for C in (0, 17):
        slots = {name: np.zeros((1, max(C, 1)), vc.SLOT_DTYPES[name]) for name in vc.SLOT_FIELDS}
        vin = awfm.verify_inputs(case.read_chars.ctypes.data, 4, case.offsets.ctypes.data, **{n: a.ctypes.data for n, a in slots.items()})
        rc = lib.awfmVerifyChains(vin, 1, C, 2, 3, case.text.ctypes.data, case.text.size, None, 0, vc.DNA, awfm.verify_outputs(), 1)
        assert rc == awfm.AwFmIllegalPositionError


def test_every_output_null_in_turn_and_the_counter_is_added_to(awfm):
    case = vc.random_case(3, 50, 4)
    want = case.host(awfm, 2, 3)
    names = ["editDistances", "bestSlots", "numUnverified"]
    for missing in names:
        for outputs in ([n for n in names if n != missing], [missing]):
            got = case.host(awfm, 2, 3, outputs=outputs, fill=0xC3)
            assert sorted(got) == sorted(outputs)
            vc.assert_equal(got, want, names=outputs, what=str(outputs))
    assert case.host(awfm, 2, 3, unverified_before=2 ** 40)["numUnverified"] == 2 ** 40 + want["numUnverified"]


def test_read_offsets_that_are_inverted_or_leave_the_buffer(awfm):
    b = vc.Builder([b"acgtacgtacgtacgt"])
    for k in range(4):
        b.add(f"read {k}", b"acgt", 0, 4, 0, 4 * k, 4 * k + 4, 0)
    case = b.case()
    case.offsets = np.array([0, 4, 3, 12, 17], np.uint64)  # read 1 inverted, read 2 fine (its chain within it), read 3 beyond the 16
    got = case.host(awfm, 2, 3)
    assert got["editDistances"][:, 0].tolist() == [0, vc.MALFORMED, vc.unbanded(b"tacg", b"acgt"), vc.MALFORMED]
    assert got["numUnverified"] == 2 and got["bestSlots"].tolist() == [0, vc.NO_SLOT, 0, vc.NO_SLOT]
    case.num_read_chars = 11  # now read 2 leaves it too
    assert case.host(awfm, 2, 3)["editDistances"][:, 0].tolist() == [0, vc.MALFORMED, vc.MALFORMED, vc.MALFORMED]


@pytest.mark.parametrize("length", [96, 97, 98, 99, 111, 112, 113])
def test_last_record_ending_at_the_texts_last_byte(awfm, length):
    b = vc.tail_case(length)
    got = b.case().host(awfm, 2, 3)
    assert np.array_equal(got["editDistances"], b.want())


def test_one_sequence_without_a_record_table_and_the_amino_alphabet(awfm):
    slots = {name: np.array([[v]], vc.SLOT_DTYPES[name]) for name, v in zip(vc.SLOT_FIELDS, (0, 1, 0, 4, 2, 2))}
    case = vc.Case(b"ARXD", [0, 4], slots, b"mkarxdmk", None, vc.AMINO)
    assert int(case.host(awfm, 1, 1)["editDistances"][0, 0]) == 1  # x matches nothing, not even itself; case is ignored
    slots["sequences"][0, 0] = 1
    assert int(vc.Case(b"ARXD", [0, 4], slots, b"mkarxdmk", None, vc.AMINO).host(awfm, 1, 1)["editDistances"][0, 0]) == vc.MALFORMED
    slots["sequences"][0, 0] = 0
    assert int(vc.Case(b"ARND", [0, 4], slots, b"mkarndmk", None, vc.AMINO).host(awfm, 1, 1)["editDistances"][0, 0]) == 0
    assert int(vc.Case(b"acgt", [0, 4], slots, b"ttACGTtt", None, vc.DNA).host(awfm, 0, 0)["editDistances"][0, 0]) == 0


def long_case():
    """a record of 2^20 + 1 characters and a read that copies it with five substitutions inside its first 2^20: slot 0 verifies
    2^20 characters (5), slot 1 one more (too long)"""
    rng = np.random.default_rng(20)
    n = vc.MAX_LENGTH
    text = rng.choice(np.frombuffer(b"acgt", np.uint8), n + 1)
    read = text.copy()
    for at in (0, 1000, n // 2, n - 2, n - 1):
        read[at] = ord("a") if read[at] != ord("a") else ord("c")
    slots = {name: np.array([[0, 0]], vc.SLOT_DTYPES[name]) for name in vc.SLOT_FIELDS}
    slots["chainAnchors"][0] = 1
    slots["chainReadEnds"][0] = (n, n + 1)
    return vc.Case(read.tobytes(), [0, n + 1], slots, text.tobytes() + b"\0", [n + 1])


def test_too_long_at_two_to_the_twenty_and_one_more(awfm):
    got = long_case().host(awfm, 8, 15)
    assert got["editDistances"].tolist() == [[5, vc.TOO_LONG]] and got["numUnverified"] == 1 and got["bestSlots"].tolist() == [0]


def test_end_to_end_on_the_host_verifies_every_planted_read_and_rejects_the_decoys(awfm, tmp_path):
    """FASTA -> longest matches -> located -> mapped -> candidates -> chains -> verification, all host twins"""
    import read_candidates_common as rc
    import read_chains_common as ch
    fa, records, reads, planted, decoy_of = vc.planted_with_decoys(str(tmp_path))
    ix = awfm.create_index_from_fasta(fa, awfm.AwFmAlphabetDna, 8, 8, file_src=str(tmp_path / "records.awfmi"))
    try:
        host = rc.host_pipeline(awfm, ix, reads)
    finally:
        ix.dealloc()
    chain_case = ch.candidate_case(awfm, host, 2, 4, max_hits_per_seed=rc.E2E_MAX_HITS, min_votes=2)
    chains = chain_case.host(awfm, max_hits_per_seed=rc.E2E_MAX_HITS, band=2, gap_penalty=1)
    text, ends = vc.text_of(records)
    slots = dict({name: chains[name] for name in vc.SLOT_FIELDS[1:]}, sequences=chain_case.sequences)
    case = vc.Case(b"".join(reads), np.arange(len(reads) + 1) * rc.E2E_READ_LENGTH, slots, text.tobytes(), ends)
    got = case.host(awfm, vc.E2E_W, vc.E2E_X)
    assert got["numUnverified"] == 0  # chains made from located hits are never malformed
    vc.assert_planted_reads_verified(case, got, planted, decoy_of)


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
  const uint64_t numReads = h[0], slots = h[1], sizeChars = h[2], textLength = h[4], numRecords = h[5], n = numReads * slots;
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
  const uint8_t *text = block(f, textLength);
  const uint64_t *ends = numRecords ? block(f, numRecords * 8) : NULL;
  uint64_t unverified = h[9];
  struct AwFmVerifyOutputs out = {malloc(n * 4), malloc(numReads * 4), &unverified};
  if (awfmVerifyChains(&in, numReads, (uint32_t)slots, (uint32_t)h[6], (uint32_t)h[7], text, textLength, ends, numRecords, (int)h[8], &out,
                       (unsigned)h[10]) != AwFmSuccess)
    return 3;
  /* the windows of the text around every read's offset, h[11] bytes before and after */
  uint8_t *windows = malloc(numReads * 2 * h[11] + 1);
  if (awfmTextWindows(text, textLength, in.readOffsets, numReads, (uint32_t)h[11], (uint32_t)h[11], windows, (unsigned)h[10]) != AwFmSuccess) return 4;
  fwrite(out.editDistances, 4, n, stdout);
  fwrite(out.bestSlots, 4, numReads, stdout);
  fwrite(&unverified, 8, 1, stdout);
  fwrite(windows, 1, numReads * 2 * h[11], stdout);
  return 0;
}
"""


def test_host_twins_under_address_and_undefined_sanitizers(awfm, tmp_path):
    """the twins index the read buffer and the text by offsets and diagonals their caller supplies: awfm_verify.c, the letter
    tables and the thread pool, compiled with a stand-alone main under -fsanitize=address,undefined, run on the edge list (every
    malformed shape in it), on the tails that end at the text's last byte and on a random batch spread over four threads, every
    array in a heap block of exactly its size"""
    (tmp_path / "main.c").write_text(SANITIZER_MAIN)
    exe = str(tmp_path / "verify_asan")
    subprocess.check_call(["gcc", "-std=gnu11", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-pthread", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, str(tmp_path / "main.c"),
                           os.path.join(CSRC, "awfm_verify.c"), os.path.join(CSRC, "awfm_letters.c"), os.path.join(CSRC, "awfm_threads.c"),
                           "-o", exe])
    cases = [("edge", vc.edge_builder(2, 3).case(), 2, 3, 2), ("edge-wide", vc.edge_builder(24, 15).case(3), 24, 15, 1),
             ("tail", vc.tail_case(113).case(), 2, 3, 1), ("random", vc.random_case(8, 400, 4, max_length=80), 4, 7, 4),
             ("amino", vc.random_case(9, 100, 16, vc.AMINO), 8, 15, 4)]
    for name, case, w, x, threads in cases:
        half = 37
        header = np.array([case.num_reads, case.C, case.read_chars.size, case.num_read_chars, case.text.size, len(case.ends), w, x, case.alphabet,
                           6, threads, half], np.uint64)
        arrays = [header, case.read_chars, case.offsets] + [case.slots[f] for f in vc.SLOT_FIELDS] + [case.text, case.ends]
        (tmp_path / name).write_bytes(b"".join(a.tobytes() for a in arrays))
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
        run = subprocess.run([exe, str(tmp_path / name)], capture_output=True, env=env, timeout=120)
        assert run.returncode == 0, (name, run.stderr.decode(errors="replace")[-3000:])
        want = case.host(awfm, w, x, unverified_before=6)
        n = case.num_reads * case.C
        assert np.array_equal(np.frombuffer(run.stdout, np.uint32, n), want["editDistances"].reshape(-1)), name
        assert np.array_equal(np.frombuffer(run.stdout, np.uint32, case.num_reads, 4 * n), want["bestSlots"]), name
        assert int(np.frombuffer(run.stdout, np.uint64, 1, 4 * n + 4 * case.num_reads)[0]) == want["numUnverified"]
        windows = np.frombuffer(run.stdout, np.uint8, case.num_reads * 2 * half, 4 * n + 4 * case.num_reads + 8)
        assert np.array_equal(windows.reshape(case.num_reads, 2 * half), awfm.text_windows_host(case.text, case.offsets[:-1], half, half))
