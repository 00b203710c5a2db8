/*
 * alignment_strings_sanitize.c -- awfmAlignmentStrings (csrc/awfm_strings.c) under AddressSanitizer and UBSan, as a stand-alone
 * program: the definition's hand values and its SKIPPED conditions, with every array in a heap block of exactly its size, so
 * that a read or a write one byte outside any of them stops the program; then 2^13 random reads on 1 and on 16 threads, whose
 * outputs must be equal.  Exit status 0: every string is the expected one.
 *
 *   cc -std=gnu11 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude -Iavxwindowfmindex_amd/csrc \
 *      scripts/alignment_strings_sanitize.c avxwindowfmindex_amd/csrc/awfm_strings.c avxwindowfmindex_amd/csrc/awfm_threads.c \
 *      -pthread -static-libasan -static-libubsan -o alignment_strings_sanitize && ./alignment_strings_sanitize
 *
 * (tests/test_alignment_strings_sanitizer.py does exactly that.)
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "AwFmIndex.h"
#include "awfm_gpu.h"

enum { I = 1, D = 2, S = 4, EQ = 7, X = 8, SLOTS = 2, MAX_OPS = 6, MAX_READS = 64 };

struct Read {
  uint32_t record, slot, sequence, numOps, ops[MAX_OPS];
  uint64_t begin;
  const char *cigar, *classic, *md; /* NULL: SKIPPED */
};

#define RUN(n, op) (((uint32_t)(n) << 4) | (op))

static int failures;

static void *exact(const void *from, size_t bytes) { /* a heap block of exactly `bytes` bytes */
  void *p = malloc(bytes ? bytes : 1);
  if (from && bytes) memcpy(p, from, bytes);
  return p;
}

static void expectString(const char *what, uint64_t r, const uint8_t *chars, const uint64_t *offsets, const char *want) {
  const uint64_t length = offsets[r + 1] - offsets[r];
  if (length != strlen(want) || memcmp(chars + offsets[r], want, length) != 0) {
    fprintf(stderr, "read %" PRIu64 " %s: got %.*s, want %s\n", r, what, (int)length, (const char *)chars + offsets[r], want);
    failures++;
  }
}

/* The threaded passes.  awfmParallelFor runs a loop of fewer than 4096 items on the calling thread, so the hand values above never
 * leave it: here 2^13 reads with random scripts, skipped reads in every stretch of eight, at capacities that hold everything, two
 * thirds and nothing -- so that overflowing reads fill whole chunks --, once on 1 thread and once on 16, every output equal byte
 * for byte.  The per-thread counters, the chunked lengths pass and the concurrent writes into the arenas run under the sanitizers. */
enum { BIG_READS = 1 << 13, BIG_OPS = 8, BIG_TEXT = 1 << 14, BIG_RECORDS = 5 };

static uint64_t lcgState = 12345;
static uint32_t lcg(uint32_t below) {
  lcgState = lcgState * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(lcgState >> 33) % below;
}

struct BigResult {
  uint64_t *cigarOffsets, *mdOffsets, counters[2];
  uint8_t *cigarChars, *mdChars;
};

static int threadedBatch(void) {
  static const uint8_t letters[] = "acgtACGTnN$\0*";
  static const uint32_t opsOf[] = {EQ, EQ, EQ, X, X, I, D, S};
  uint8_t *text = exact(NULL, BIG_TEXT);
  for (uint64_t i = 0; i < BIG_TEXT; i++) text[i] = letters[lcg(sizeof letters - 1)];
  uint64_t *ends = exact(NULL, BIG_RECORDS * 8);
  for (uint64_t s = 0; s < BIG_RECORDS; s++) ends[s] = (s + 1) * (BIG_TEXT / BIG_RECORDS) - 1;
  const uint64_t recordLength = BIG_TEXT / BIG_RECORDS - 1; /* every record but the first; the first has one more */
  uint32_t *sequences = exact(NULL, (size_t)BIG_READS * SLOTS * 4), *slots = exact(NULL, BIG_READS * 4), *numOps = exact(NULL, BIG_READS * 4);
  uint32_t *ops = exact(NULL, (size_t)BIG_READS * BIG_OPS * 4);
  uint64_t *begins = exact(NULL, BIG_READS * 8), wantSkipped = 0;
  for (uint64_t r = 0; r < BIG_READS; r++) {
    const uint32_t k = r % 11 == 0 ? 0 : 1 + lcg(BIG_OPS), slot = lcg(SLOTS);
    uint64_t textLength = 0;
    for (uint32_t i = 0; i < BIG_OPS; i++) {
      const uint32_t len = 1 + lcg(lcg(4) ? 3 : 40), op = opsOf[lcg(8)];
      ops[r * BIG_OPS + i] = RUN(len, op);
      if (i < k && (op == EQ || op == X || op == D)) textLength += len;
    }
    for (int j = 0; j < SLOTS; j++) sequences[r * SLOTS + j] = 0xFFFFFFFEu;
    sequences[r * SLOTS + slot] = lcg(BIG_RECORDS);
    slots[r] = slot;
    numOps[r] = k;
    begins[r] = lcg((uint32_t)(recordLength - textLength));
    if (k != 0 && r % 8 == 3) { /* a skipped read in every stretch of eight, four kinds in turn */
      const uint32_t kind = (uint32_t)(r / 8) % 4;
      if (kind == 0) slots[r] = 0xFFFFFFFFu;
      else if (kind == 1) sequences[r * SLOTS + slot] = BIG_RECORDS + lcg(3);
      else if (kind == 2) begins[r] = recordLength + 2 + lcg(9);
      else ops[r * BIG_OPS + k - 1] = RUN(lcg(3), 3);
      wantSkipped++;
    }
  }
  const struct AwFmStringInputs in = {.sequences = sequences, .slots = slots, .textBegins = begins, .numOps = numOps, .ops = ops};
  int bad = 0;
  for (uint32_t flags = 0; flags <= AWFM_STRINGS_CIGAR_M; flags++) {
    uint64_t totals[2] = {0, 0};
    for (int share = 3; share >= 0; share -= (share == 3 ? 1 : 2)) { /* capacities: the totals, two thirds of them, nothing */
      struct BigResult result[2];
      for (int side = 0; side < 2; side++) {
        struct BigResult *b = &result[side];
        b->cigarOffsets = exact(NULL, (BIG_READS + 1) * 8);
        b->mdOffsets = exact(NULL, (BIG_READS + 1) * 8);
        b->counters[0] = 7;
        b->counters[1] = 9;
        struct AwFmStringOutputs out = {.cigarOffsets = b->cigarOffsets, .mdOffsets = b->mdOffsets};
        const unsigned threads = side ? 16 : 1;
        if (awfmAlignmentStrings(&in, BIG_READS, SLOTS, BIG_OPS, flags, text, BIG_TEXT, ends, BIG_RECORDS, AwFmAlphabetDna, &out, threads) != AwFmSuccess) return 1;
        totals[0] = b->cigarOffsets[BIG_READS];
        totals[1] = b->mdOffsets[BIG_READS];
        out.cigarCapacity = totals[0] * (uint64_t)share / 3;
        out.mdCapacity = totals[1] * (uint64_t)share / 3;
        out.cigarChars = b->cigarChars = exact(NULL, out.cigarCapacity);
        out.mdChars = b->mdChars = exact(NULL, out.mdCapacity);
        memset(b->cigarChars, 0x5A, out.cigarCapacity ? out.cigarCapacity : 1);
        memset(b->mdChars, 0x5A, out.mdCapacity ? out.mdCapacity : 1);
        out.numSkipped = &b->counters[0];
        out.numOverflow = &b->counters[1];
        if (awfmAlignmentStrings(&in, BIG_READS, SLOTS, BIG_OPS, flags, text, BIG_TEXT, ends, BIG_RECORDS, AwFmAlphabetDna, &out, threads) != AwFmSuccess) return 1;
      }
      const uint64_t cigarCapacity = totals[0] * (uint64_t)share / 3, mdCapacity = totals[1] * (uint64_t)share / 3;
      if (memcmp(result[0].cigarOffsets, result[1].cigarOffsets, (BIG_READS + 1) * 8) || memcmp(result[0].mdOffsets, result[1].mdOffsets, (BIG_READS + 1) * 8) ||
          memcmp(result[0].cigarChars, result[1].cigarChars, cigarCapacity) || memcmp(result[0].mdChars, result[1].mdChars, mdCapacity) ||
          result[0].counters[0] != result[1].counters[0] || result[0].counters[1] != result[1].counters[1]) {
        fprintf(stderr, "2^13 reads, flags %u, capacities %d/3: 1 and 16 threads differ\n", flags, share);
        bad++;
      }
      /* what must hold whatever the threads: the skipped reads, and at capacity 0 every read with strings overflows */
      uint64_t withStrings = 0;
      for (uint64_t r = 0; r < BIG_READS; r++) withStrings += result[1].cigarOffsets[r + 1] > result[1].cigarOffsets[r];
      if (result[1].counters[0] != 7 + wantSkipped || (share == 3 && result[1].counters[1] != 9) || (share == 0 && result[1].counters[1] != 9 + withStrings) ||
          (share == 2 && (result[1].counters[1] <= 9 + withStrings / 4 || result[1].counters[1] >= 9 + withStrings))) {
        fprintf(stderr, "2^13 reads, flags %u, capacities %d/3: counters %" PRIu64 " %" PRIu64 " (%" PRIu64 " skipped, %" PRIu64 " with strings)\n", flags, share,
                result[1].counters[0], result[1].counters[1], wantSkipped, withStrings);
        bad++;
      }
      for (int side = 0; side < 2; side++) {
        free(result[side].cigarOffsets);
        free(result[side].mdOffsets);
        free(result[side].cigarChars);
        free(result[side].mdChars);
      }
    }
  }
  free(text);
  free(ends);
  free(sequences);
  free(slots);
  free(numOps);
  free(ops);
  free(begins);
  if (!bad) printf("alignment strings: %d reads, %" PRIu64 " skipped, both forms, three capacities: 1 and 16 threads agree\n", (int)BIG_READS, wantSkipped);
  return bad;
}

int main(void) {
  /* the records of the definition's table, each followed by a terminator */
  static const char *const records[] = {"ACGTACGTAC", "TTGGGGG", "AAAAAg", "AAAAAAAAAA", "a\0C", "ACGTACGT"};
  static const size_t lengths[] = {10, 7, 6, 10, 3, 8};
  enum { RECORDS = 6 };
  uint8_t text[64];
  uint64_t ends[RECORDS], length = 0;
  for (int s = 0; s < RECORDS; s++) {
    memcpy(text + length, records[s], lengths[s]);
    length += lengths[s];
    ends[s] = length;
    text[length++] = '$';
  }
  const uint64_t hugeBegin = UINT64_MAX - 2;
  const struct Read reads[] = {
      {0, 0, 0, 6, {RUN(2, S), RUN(3, EQ), RUN(1, X), RUN(2, I), RUN(1, D), RUN(2, EQ)}, 1, "2S3=1X2I1D2=", "2S4M2I1D2M", "3A0^C2"},
      {1, 1, 1, 2, {RUN(2, X), RUN(5, EQ)}, 0, "2X5=", "7M", "0T0T5"},
      {2, 0, 2, 2, {RUN(5, EQ), RUN(1, X)}, 0, "5=1X", "6M", "5G0"},
      {3, 1, 3, 3, {RUN(9, EQ), RUN(1, I), RUN(1, EQ)}, 0, "9=1I1=", "9M1I1M", "10"},
      {4, 0, 4, 3, {RUN(1, D), RUN(1, X), RUN(1, EQ)}, 0, "1D1X1=", "1D2M", "0^A0N1"},
      {5, 1, 5, 5, {RUN(3, EQ), RUN(2, D), RUN(1, I), RUN(2, D), RUN(1, EQ)}, 0, "3=2D1I2D1=", "3M2D1I2D1M", "3^TA0^CG1"},
      /* NONE: nothing else of the read is looked at */
      {9, 77, 9, 0, {0}, hugeBegin, "", "", ""},
      /* SKIPPED, each beside reads that are fine */
      {0, 0, 0, MAX_OPS + 1, {RUN(1, EQ)}, 0, NULL, NULL, NULL},             /* a truncated row */
      {0, SLOTS, 0, 1, {RUN(1, EQ)}, 0, NULL, NULL, NULL},                   /* j >= C */
      {0, 0xFFFFFFFFu, 0, 1, {RUN(1, EQ)}, 0, NULL, NULL, NULL},             /* AWFM_CHAINS_NO_SLOT */
      {0, 0, RECORDS, 1, {RUN(1, EQ)}, 0, NULL, NULL, NULL},                 /* s >= numRecords */
      {0, 0, 0xFFFFFFFFu, 1, {RUN(1, EQ)}, 0, NULL, NULL, NULL},
      {0, 0, 0, 2, {RUN(1, EQ), RUN(0, X)}, 0, NULL, NULL, NULL},            /* a run without a length */
      {0, 0, 0, 2, {RUN(1, EQ), RUN(1, 0)}, 0, NULL, NULL, NULL},            /* M is no operation of a script */
      {0, 0, 0, 2, {RUN(1, EQ), RUN(1, 15)}, 0, NULL, NULL, NULL},
      {0, 0, 0, 2, {RUN(65536, S), RUN(1, I)}, 0, NULL, NULL, NULL},         /* read length 2^16 + 1 */
      {0, 0, 0, 2, {RUN(131072, D), RUN(1, X)}, 0, NULL, NULL, NULL},        /* text length 2^17 + 1 */
      {0, 0, 0, 6, {RUN(0xFFFFFFF, EQ), RUN(0xFFFFFFF, EQ), RUN(0xFFFFFFF, EQ), RUN(0xFFFFFFF, D), RUN(0xFFFFFFF, D), RUN(0xFFFFFFF, D)}, 0, NULL, NULL, NULL},
      {0, 0, 0, 1, {RUN(1, S)}, 11, NULL, NULL, NULL},                       /* textBegin > L */
      {0, 0, 0, 1, {RUN(3, X)}, 8, NULL, NULL, NULL},                        /* one position past the record's end */
      {5, 0, 5, 2, {RUN(7, EQ), RUN(2, D)}, 0, NULL, NULL, NULL},            /* ... of the last record: past the text itself */
      {0, 0, 0, 1, {RUN(1, EQ)}, hugeBegin, NULL, NULL, NULL},               /* textBegin near 2^64 */
      /* valid at the very end of a record, and of the text */
      {0, 0, 0, 1, {RUN(3, X)}, 7, "3X", "3M", "0T0A0C0"},
      {5, 0, 5, 2, {RUN(6, EQ), RUN(2, D)}, 0, "6=2D", "6M2D", "6^GT0"},
      {0, 0, 0, 1, {RUN(4, S)}, 10, "4S", "4S", "0"},
  };
  const uint64_t n = sizeof reads / sizeof *reads;
  uint32_t sequences[MAX_READS * SLOTS], slots[MAX_READS], numOps[MAX_READS], ops[MAX_READS * MAX_OPS];
  uint64_t begins[MAX_READS], wantSkipped = 0;
  for (uint64_t r = 0; r < n; r++) {
    for (int j = 0; j < SLOTS; j++) sequences[r * SLOTS + j] = 0xFFFFFFFEu;
    if (reads[r].slot < SLOTS) sequences[r * SLOTS + reads[r].slot] = reads[r].sequence;
    slots[r] = reads[r].slot;
    numOps[r] = reads[r].numOps;
    begins[r] = reads[r].begin;
    memcpy(ops + r * MAX_OPS, reads[r].ops, sizeof reads[r].ops);
    wantSkipped += reads[r].cigar == NULL;
  }
  /* (the text without its last terminator: the last record ends where the text does) */
  const uint64_t textLength = length - 1;
  const struct AwFmStringInputs in = {.sequences = exact(sequences, n * SLOTS * 4), .slots = exact(slots, n * 4), .textBegins = exact(begins, n * 8),
                                      .numOps = exact(numOps, n * 4), .ops = exact(ops, n * MAX_OPS * 4)};
  uint8_t *exactText = exact(text, textLength);
  uint64_t *exactEnds = exact(ends, sizeof ends);
  for (unsigned threads = 1; threads <= 16; threads += 15) { /* (a batch this small stays on the calling thread either way: see threadedBatch) */
    for (uint32_t flags = 0; flags <= AWFM_STRINGS_CIGAR_M; flags++) {
      uint64_t *cigarOffsets = exact(NULL, (n + 1) * 8), *mdOffsets = exact(NULL, (n + 1) * 8), counters[2] = {100, 200};
      struct AwFmStringOutputs out = {.cigarOffsets = cigarOffsets, .mdOffsets = mdOffsets};
      enum AwFmReturnCode rc = awfmAlignmentStrings(&in, n, SLOTS, MAX_OPS, flags, exactText, textLength, exactEnds, RECORDS, AwFmAlphabetDna, &out, threads);
      if (rc != AwFmSuccess) return 2;
      /* arenas of exactly the totals; then of one byte less: the last strings are left out, and nothing is written beyond */
      for (uint64_t less = 0; less <= 1; less++) {
        out.cigarCapacity = cigarOffsets[n] - less;
        out.mdCapacity = mdOffsets[n] - less;
        out.cigarChars = exact(NULL, out.cigarCapacity);
        out.mdChars = exact(NULL, out.mdCapacity);
        out.numSkipped = &counters[0];
        out.numOverflow = &counters[1];
        counters[0] = 100;
        counters[1] = 200;
        rc = awfmAlignmentStrings(&in, n, SLOTS, MAX_OPS, flags, exactText, textLength, exactEnds, RECORDS, AwFmAlphabetDna, &out, threads);
        if (rc != AwFmSuccess) return 2;
        if (counters[0] != 100 + wantSkipped || counters[1] != 200 + less) {
          fprintf(stderr, "counters %" PRIu64 " %" PRIu64 ", want %" PRIu64 " %" PRIu64 "\n", counters[0], counters[1], 100 + wantSkipped, 200 + less);
          failures++;
        }
        for (uint64_t r = 0; r + less < n; r++) { /* (with one byte less the last read, which has strings, is not written) */
          expectString("CIGAR", r, out.cigarChars, cigarOffsets, reads[r].cigar ? (flags ? reads[r].classic : reads[r].cigar) : "");
          expectString("MD", r, out.mdChars, mdOffsets, reads[r].md ? reads[r].md : "");
        }
        free(out.cigarChars);
        free(out.mdChars);
      }
      free(cigarOffsets);
      free(mdOffsets);
    }
  }
  free((void *)in.sequences);
  free((void *)in.slots);
  free((void *)in.textBegins);
  free((void *)in.numOps);
  free((void *)in.ops);
  free(exactText);
  free(exactEnds);
  if (failures) return 1;
  printf("alignment strings: %" PRIu64 " reads, %" PRIu64 " skipped, both forms: as expected\n", n, wantSkipped);
  return threadedBatch() ? 1 : 0;
}
