/*
 * sam_records_sanitize.c -- awfmSamRecords, awfmRecordNames and awfmSamHeader (csrc/awfm_sam.c) under AddressSanitizer and UBSan,
 * as a stand-alone program: lines written out by hand -- pairs in every combination, every reason a read is unaligned, reads of
 * length 0, empty strings, every optional array NULL --, with every array in a heap block of exactly its size, so that a read or
 * a write one byte outside any of them stops the program; the capacities; then 2^13 random reads on 1 and on 16 threads, whose
 * outputs must be equal.  Exit status 0: every line is the expected one.
 *
 *   cc -std=gnu11 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude -Iavxwindowfmindex_amd/csrc \
 *      scripts/sam_records_sanitize.c avxwindowfmindex_amd/csrc/awfm_sam.c avxwindowfmindex_amd/csrc/awfm_threads.c \
 *      -pthread -static-libasan -static-libubsan -o sam_records_sanitize && ./sam_records_sanitize
 *
 * (tests/test_sam_records_sanitizer.py does exactly that.)
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "AwFmIndex.h"
#include "awfm_gpu.h"
#include "awfm_internal.h"

enum { SLOTS = 2, MAX_READS = 16 };

struct Read {
  const char *seq, *qual, *name, *cigar, *md;
  uint32_t score, nm, slot, records[SLOTS], xs;
  uint64_t begin, end;
  uint8_t mapq;
  uint16_t flag;
  int inverted;                 /* its end offset lies one byte before its begin */
  const char *paired, *single; /* the lines: as mates with every array, alone with every optional array NULL */
};

static int failures;

static void *exact(const void *from, size_t bytes) { /* a heap block of exactly `bytes` bytes */
  void *p = malloc(bytes ? bytes : 1);
  if (from && bytes) memcpy(p, from, bytes);
  return p;
}

static const char *recordNames[4] = {"chr1", "r2", "", "long_name|x"};

static const struct Read hand[] = {
    {"ACGTA", "IIII#", "pair", "5M", "5", 5, 0, 0, {0, 1}, 3, 99, 104, 60, 0, 0,
     "pair\t99\tchr1\t100\t60\t5M\t=\t300\t205\tACGTA\tIIII#\tNM:i:0\tAS:i:5\tXS:i:3\tMD:Z:5\n",
     "0\t0\tchr1\t100\t255\t5M\t*\t0\t0\tACGTA\t*\tNM:i:0\tAS:i:5\n"},
    {"TTGCA", "#IIII", "pair", "2M1X2M", "2C2", 4, 1, 0, {0, 1}, 0, 299, 304, 9, 0x10, 0,
     "pair\t147\tchr1\t300\t9\t2M1X2M\t=\t100\t-205\tTTGCA\t#IIII\tNM:i:1\tAS:i:4\tXS:i:0\tMD:Z:2C2\n",
     "1\t0\tchr1\t300\t255\t2M1X2M\t*\t0\t0\tTTGCA\t*\tNM:i:1\tAS:i:4\n"},
    {"GG", "!!", "lone", "2M", "2", 0, 0, 0, {0, 1}, 0, 4, 6, 60, 0, 0, "lone\t69\tr2\t10\t0\t*\t=\t10\t0\tGG\t!!\n", "2\t4\t*\t0\t0\t*\t*\t0\t0\tGG\t*\n"},
    {"", "", "mate", "", "", 2, 0, 0, {1, 0}, 0, 9, 9, 60, 0, 0, "mate\t137\tr2\t10\t60\t*\t*\t0\t0\t*\t*\tNM:i:0\tAS:i:2\tXS:i:0\n",
     "3\t0\tr2\t10\t255\t*\t*\t0\t0\t*\t*\tNM:i:0\tAS:i:2\n"},
    /* two records: RNEXT is a name, TLEN 0; 2^40 and the largest values */
    {"AC", "ab", "two", "2M", "2", 0xFFFFFFFBu, 0xFFFFFFFFu, 1, {9, 3}, 0xFFFFFFFFu, (1ull << 40) - 1, 1ull << 40, 255, 4095, 0,
     "two\t4095\tlong_name|x\t1099511627776\t255\t2M\tchr1\t1\t0\tAC\tab\tNM:i:4294967295\tAS:i:4294967291\tXS:i:4294967295\tMD:Z:2\n",
     "4\t0\tlong_name|x\t1099511627776\t255\t2M\t*\t0\t0\tAC\t*\tNM:i:4294967295\tAS:i:4294967291\n"},
    {"T", "c", "two", "1M", "1", 1, 0, 0, {0, 0}, 0, 0, 1, 0, 0, 0, "two\t163\tchr1\t1\t0\t1M\tlong_name|x\t1099511627776\t0\tT\tc\tNM:i:0\tAS:i:1\tXS:i:0\tMD:Z:1\n",
     "5\t0\tchr1\t1\t255\t1M\t*\t0\t0\tT\t*\tNM:i:0\tAS:i:1\n"},
    /* unaligned: too long, no slot; both mates unaligned */
    {"ACG", "abc", "none", "3M", "3", 0xFFFFFFFCu, 0, 0, {0, 1}, 0, 4, 7, 60, 0, 0, "none\t77\t*\t0\t0\t*\t*\t0\t0\tACG\tabc\n", "6\t4\t*\t0\t0\t*\t*\t0\t0\tACG\t*\n"},
    {"ACGT", "abcd", "none", "4M", "4", 7, 0, 0xFFFFFFFFu, {0, 1}, 0, 4, 8, 60, 0, 0, "none\t141\t*\t0\t0\t*\t*\t0\t0\tACGT\tabcd\n",
     "7\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\t*\n"},
    /* a slot of C, a record that has no name */
    {"A", "a", "x", "1M", "1", 7, 0, 2, {0, 1}, 0, 4, 5, 60, 0, 0, "x\t77\t*\t0\t0\t*\t*\t0\t0\tA\ta\n", "8\t4\t*\t0\t0\t*\t*\t0\t0\tA\t*\n"},
    {"C", "b", "x", "1M", "1", 7, 0, 0, {4, 1}, 0, 4, 5, 60, 0, 0, "x\t141\t*\t0\t0\t*\t*\t0\t0\tC\tb\n", "9\t4\t*\t0\t0\t*\t*\t0\t0\tC\t*\n"},
    /* inverted read offsets: unaligned, a read of length 0; its mate reaches one byte back; the tie on textBegins */
    {"ACGTA", "abcde", "inv", "5M", "5", 7, 0, 0, {0, 1}, 0, 4, 9, 60, 0, 1, "inv\t69\tchr1\t5\t0\t*\t=\t5\t0\t*\t*\n", "10\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\n"},
    {"GT", "fg", "inv", "3M", "3", 7, 0, 0, {0, 1}, 0, 4, 7, 60, 0, 0, "inv\t137\tchr1\t5\t60\t3M\t*\t0\t0\tCACGTAGT\tbabcdefg\tNM:i:0\tAS:i:7\tXS:i:0\tMD:Z:3\n",
     "11\t0\tchr1\t5\t255\t3M\t*\t0\t0\tCACGTAGT\t*\tNM:i:0\tAS:i:7\n"},
    {"ACGTA", "abcde", "tie", "5M", "", 7, 2, 0, {1, 1}, 0, 50, 55, 60, 0, 0, "tie\t67\tr2\t51\t60\t5M\t=\t51\t7\tACGTA\tabcde\tNM:i:2\tAS:i:7\tXS:i:0\n",
     "12\t0\tr2\t51\t255\t5M\t*\t0\t0\tACGTA\t*\tNM:i:2\tAS:i:7\n"},
    {"ACGTACG", "abcdefg", "tie", "", "7", 7, 0, 0, {1, 1}, 0, 50, 57, 60, 0, 0, "tie\t131\tr2\t51\t60\t*\t=\t51\t-7\tACGTACG\tabcdefg\tNM:i:0\tAS:i:7\tXS:i:0\tMD:Z:7\n",
     "13\t0\tr2\t51\t255\t*\t*\t0\t0\tACGTACG\t*\tNM:i:0\tAS:i:7\n"},
};
enum { HAND_READS = sizeof hand / sizeof *hand };

struct Arrays {
  struct AwFmSamInputs in;
  void *blocks[32];
  int numBlocks;
};

static void *keep(struct Arrays *a, void *block) {
  a->blocks[a->numBlocks++] = block;
  return block;
}

/* `strings[i]` back to back behind offsets, each in a block of exactly its size */
static void pack(struct Arrays *a, const char *const *strings, uint64_t n, const uint64_t **offsetsOut, const uint8_t **charsOut) {
  uint64_t *offsets = malloc((n + 1) * 8), total = 0;
  for (uint64_t i = 0; i < n; i++) total += strlen(strings[i]);
  uint8_t *chars = malloc(total ? total : 1);
  offsets[0] = 0;
  for (uint64_t i = 0; i < n; i++) {
    memcpy(chars + offsets[i], strings[i], strlen(strings[i]));
    offsets[i + 1] = offsets[i] + strlen(strings[i]);
  }
  *offsetsOut = keep(a, offsets);
  *charsOut = keep(a, chars);
}

static void build(struct Arrays *a, const struct Read *reads, uint64_t n, int all) {
  memset(a, 0, sizeof *a);
  const char *seqs[MAX_READS], *quals[MAX_READS], *names[MAX_READS], *cigars[MAX_READS], *mds[MAX_READS];
  uint32_t sequences[MAX_READS * SLOTS], slots[MAX_READS], scores[MAX_READS], nms[MAX_READS], xs[MAX_READS];
  uint64_t begins[MAX_READS], ends[MAX_READS];
  uint8_t mapqs[MAX_READS], proper[MAX_READS / 2];
  uint16_t flags[MAX_READS];
  for (uint64_t r = 0; r < n; r++) {
    seqs[r] = reads[r].seq, quals[r] = reads[r].qual, names[r] = reads[r].name, cigars[r] = reads[r].cigar, mds[r] = reads[r].md;
    memcpy(sequences + r * SLOTS, reads[r].records, sizeof reads[r].records);
    slots[r] = reads[r].slot, scores[r] = reads[r].score, nms[r] = reads[r].nm, xs[r] = reads[r].xs;
    begins[r] = reads[r].begin, ends[r] = reads[r].end, mapqs[r] = reads[r].mapq, flags[r] = reads[r].flag;
    proper[r / 2] = 1;
  }
  const uint64_t *unused;
  const uint8_t *qualities;
  pack(a, seqs, n, &a->in.readOffsets, &a->in.readChars);
  for (uint64_t r = 0; r < n; r++)
    if (reads[r].inverted) ((uint64_t *)a->in.readOffsets)[r + 1] = a->in.readOffsets[r] - 1;
  a->in.numReadChars = a->in.readOffsets[n];
  pack(a, quals, n, &unused, &qualities);
  pack(a, recordNames, 4, &a->in.recordNameOffsets, &a->in.recordNameChars);
  a->in.numRecordNames = 4;
  pack(a, cigars, n, &a->in.cigarOffsets, &a->in.cigarChars);
  a->in.sequences = keep(a, exact(sequences, n * SLOTS * 4));
  a->in.slots = keep(a, exact(slots, n * 4));
  a->in.scores = keep(a, exact(scores, n * 4));
  a->in.editDistances = keep(a, exact(nms, n * 4));
  a->in.textBegins = keep(a, exact(begins, n * 8));
  a->in.textEnds = keep(a, exact(ends, n * 8));
  if (!all) return;
  a->in.qualities = qualities;
  pack(a, names, n, &a->in.nameOffsets, &a->in.nameChars);
  pack(a, mds, n, &a->in.mdOffsets, &a->in.mdChars);
  a->in.mappingQualities = keep(a, exact(mapqs, n));
  a->in.secondScores = keep(a, exact(xs, n * 4));
  a->in.baseFlags = keep(a, exact(flags, n * 2));
  a->in.properPairs = keep(a, exact(proper, n / 2));
}

static void release(struct Arrays *a) {
  for (int i = 0; i < a->numBlocks; i++) free(a->blocks[i]);
}

static void checkHand(int paired) {
  struct Arrays a;
  build(&a, hand, HAND_READS, paired);
  uint64_t *offsets = malloc((HAND_READS + 1) * 8), counters[2] = {10, 20}, total = 0, wantUnaligned = 0;
  for (uint64_t r = 0; r < HAND_READS; r++) total += strlen(paired ? hand[r].paired : hand[r].single);
  for (uint64_t r = 0; r < HAND_READS; r++) wantUnaligned += strstr(paired ? hand[r].paired : hand[r].single, "\tNM:i:") == NULL; /* only aligned reads have tags */
  /* offsets alone, then the arena at three capacities, each arena a block of exactly the capacity */
  struct AwFmSamOutputs out = {.lineOffsets = offsets};
  if (awfmSamRecords(&a.in, HAND_READS, SLOTS, paired ? AWFM_SAM_PAIRED : 0, &out, 1) != AwFmSuccess || offsets[HAND_READS] != total) {
    fprintf(stderr, "sizing: %" PRIu64 " bytes, want %" PRIu64 "\n", offsets[HAND_READS], total);
    failures++;
  }
  const uint64_t capacities[3] = {total, total - 1, offsets[5] + 3};
  for (int c = 0; c < 3 && !failures; c++) {
    uint8_t *arena = malloc(capacities[c] ? capacities[c] : 1);
    memset(arena, '#', capacities[c]);
    out = (struct AwFmSamOutputs){.lineOffsets = offsets, .lineChars = arena, .lineCapacity = capacities[c], .numUnaligned = &counters[0],
                                  .numOverflow = &counters[1]};
    counters[0] = 10, counters[1] = 20;
    if (awfmSamRecords(&a.in, HAND_READS, SLOTS, paired ? AWFM_SAM_PAIRED : 0, &out, 3) != AwFmSuccess) failures++;
    uint64_t overflow = 0;
    for (uint64_t r = 0; r < HAND_READS; r++) {
      const char *want = paired ? hand[r].paired : hand[r].single;
      const uint64_t length = offsets[r + 1] - offsets[r];
      if (offsets[r + 1] > capacities[c]) {
        overflow++;
        for (uint64_t i = offsets[r]; i < capacities[c]; i++)
          if (arena[i] != '#') failures++, fprintf(stderr, "read %" PRIu64 ": a byte of a line that does not fit\n", r);
        continue;
      }
      if (length != strlen(want) || memcmp(arena + offsets[r], want, length) != 0) {
        fprintf(stderr, "read %" PRIu64 " (%s): got %.*s want %s", r, paired ? "paired" : "single", (int)length, (const char *)arena + offsets[r], want);
        failures++;
      }
    }
    if (counters[0] != 10 + wantUnaligned || counters[1] != 20 + overflow) {
      fprintf(stderr, "counters %" PRIu64 " %" PRIu64 ", want %" PRIu64 " %" PRIu64 "\n", counters[0], counters[1], 10 + wantUnaligned, 20 + overflow);
      failures++;
    }
    free(arena);
  }
  if (!failures) printf("sam records: %d reads %s, %" PRIu64 " unaligned, three capacities: as expected\n", (int)HAND_READS, paired ? "paired" : "single", wantUnaligned);
  free(offsets);
  release(&a);
}

/* The threaded passes.  awfmParallelFor runs a loop of fewer than 4096 items on the calling thread: here 2^13 random reads, pairs,
 * at capacities that hold everything, two thirds and nothing, once on 1 thread and once on 16, every output equal byte for byte. */
enum { BIG_READS = 1 << 13 };

static uint64_t lcgState = 12345;
static uint32_t lcg(uint32_t below) {
  lcgState = lcgState * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(lcgState >> 33) % below;
}

static void checkThreads(void) {
  const uint64_t n = BIG_READS;
  uint64_t *readOffsets = malloc((n + 1) * 8), *stringOffsets = malloc((n + 1) * 8), *begins = malloc(n * 8), *ends = malloc(n * 8);
  uint32_t *sequences = malloc(n * SLOTS * 4), *slots = malloc(n * 4), *scores = malloc(n * 4), *nms = malloc(n * 4);
  uint16_t *flags = malloc(n * 2);
  uint8_t *proper = malloc(n / 2);
  readOffsets[0] = stringOffsets[0] = 0;
  for (uint64_t r = 0; r < n; r++) {
    readOffsets[r + 1] = readOffsets[r] + lcg(40);
    stringOffsets[r + 1] = stringOffsets[r] + lcg(9);
    begins[r] = (uint64_t)lcg(1u << 30) << lcg(11);
    ends[r] = begins[r] + lcg(60);
    sequences[r * SLOTS] = lcg(5), sequences[r * SLOTS + 1] = lcg(4);
    slots[r] = lcg(3), scores[r] = lcg(8) ? lcg(1u << 20) : 0, nms[r] = lcg(1000), flags[r] = (uint16_t)lcg(4096);
    proper[r / 2] = (uint8_t)lcg(2);
  }
  uint8_t *chars = malloc(readOffsets[n] + 1), *strings = malloc(stringOffsets[n] + 1);
  for (uint64_t i = 0; i < readOffsets[n]; i++) chars[i] = (uint8_t)"ACGTN"[lcg(5)];
  for (uint64_t i = 0; i < stringOffsets[n]; i++) strings[i] = (uint8_t)('0' + lcg(10));
  struct Arrays names;
  memset(&names, 0, sizeof names);
  const uint64_t *nameOffsets;
  const uint8_t *nameChars;
  pack(&names, recordNames, 4, &nameOffsets, &nameChars);
  const struct AwFmSamInputs in = {.readChars = chars, .numReadChars = readOffsets[n], .readOffsets = readOffsets, .qualities = chars,
                                   .recordNameOffsets = nameOffsets, .recordNameChars = nameChars, .numRecordNames = 4, .sequences = sequences,
                                   .slots = slots, .scores = scores, .editDistances = nms, .textBegins = begins, .textEnds = ends,
                                   .cigarOffsets = stringOffsets, .cigarChars = strings, .mdOffsets = stringOffsets, .mdChars = strings,
                                   .secondScores = nms, .baseFlags = flags, .properPairs = proper};
  uint64_t *sized = malloc((n + 1) * 8);
  struct AwFmSamOutputs out = {.lineOffsets = sized};
  if (awfmSamRecords(&in, n, SLOTS, AWFM_SAM_PAIRED, &out, 16) != AwFmSuccess) failures++;
  const uint64_t total = sized[n], capacities[3] = {total, total * 2 / 3, 0};
  int bad = 0;
  for (int c = 0; c < 3; c++) {
    uint8_t *arenas[2];
    uint64_t *offsets[2], counters[2][2] = {{1, 2}, {1, 2}};
    for (int t = 0; t < 2; t++) {
      arenas[t] = memset(malloc(capacities[c] ? capacities[c] : 1), '#', capacities[c] ? capacities[c] : 1);
      offsets[t] = malloc((n + 1) * 8);
      out = (struct AwFmSamOutputs){.lineOffsets = offsets[t], .lineChars = arenas[t], .lineCapacity = capacities[c], .numUnaligned = &counters[t][0],
                                    .numOverflow = &counters[t][1]};
      if (awfmSamRecords(&in, n, SLOTS, AWFM_SAM_PAIRED, &out, t ? 16 : 1) != AwFmSuccess) bad++;
    }
    bad += memcmp(offsets[0], offsets[1], (n + 1) * 8) != 0 || memcmp(offsets[0], sized, (n + 1) * 8) != 0;
    bad += memcmp(arenas[0], arenas[1], capacities[c]) != 0 || memcmp(counters[0], counters[1], sizeof counters[0]) != 0;
    uint64_t overflow = 0;
    for (uint64_t r = 0; r < n; r++) overflow += sized[r + 1] > capacities[c];
    bad += counters[0][1] != 2 + overflow || counters[0][0] <= 1;
    for (int t = 0; t < 2; t++) free(arenas[t]), free(offsets[t]);
  }
  failures += bad;
  if (!bad) printf("sam records: %d reads, %" PRIu64 " bytes, three capacities: 1 and 16 threads agree\n", (int)BIG_READS, total);
  void *all[] = {readOffsets, stringOffsets, begins, ends, sequences, slots, scores, nms, flags, proper, chars, strings, sized};
  for (size_t i = 0; i < sizeof all / sizeof *all; i++) free(all[i]);
  release(&names);
}

/* the two helpers on a record table made by hand: headers with descriptions, blanks, a tab; blocks of exactly the sizes */
static void checkHeader(void) {
  static const char headers[] = "chr1 Homo sapiens chromosome 1scaffold_2\tlength=9lonely  leading blanks";
  const size_t headerEnds[4] = {30, 49, 55, sizeof headers - 1}, sequenceEnds[4] = {14, 24, 43, 46};
  struct FastaVector fv = {.headers = exact(headers, sizeof headers - 1), .headerLength = sizeof headers - 1, .numRecords = 4};
  struct AwfmFastaRecord records[4];
  for (int i = 0; i < 4; i++) records[i] = (struct AwfmFastaRecord){.headerEndPosition = headerEnds[i], .sequenceEndPosition = sequenceEnds[i]};
  fv.records = exact(records, sizeof records);
  struct AwFmIndex index;
  memset(&index, 0, sizeof index);
  index.fastaVector = &fv;
  static const char wantNames[] = "chr1scaffold_2lonelyleading";
  static const char want[] = "@HD\tVN:1.6\tSO:unknown\n@SQ\tSN:chr1\tLN:14\n@SQ\tSN:scaffold_2\tLN:9\n@SQ\tSN:lonely\tLN:18\n@SQ\tSN:leading\tLN:2\n";
  uint64_t *offsets = malloc(5 * 8);
  if (awfmRecordNames(&index, offsets, NULL, 0) != AwFmSuccess || offsets[4] != sizeof wantNames - 1) failures++;
  for (uint64_t capacity = 0; capacity <= offsets[4]; capacity++) {
    uint8_t *chars = malloc(capacity ? capacity : 1);
    if (awfmRecordNames(&index, offsets, chars, capacity) != AwFmSuccess) failures++;
    for (int i = 0; i < 4; i++)
      if (offsets[i + 1] <= capacity && memcmp(chars + offsets[i], wantNames + offsets[i], offsets[i + 1] - offsets[i]) != 0) failures++;
    free(chars);
  }
  if (awfmSamHeader(&index, NULL, 0) != sizeof want - 1) failures++;
  for (uint64_t capacity = 0; capacity < sizeof want; capacity++) {
    uint8_t *chars = memset(malloc(capacity ? capacity : 1), '#', capacity ? capacity : 1);
    if (awfmSamHeader(&index, chars, capacity) != sizeof want - 1) failures++;
    uint64_t whole = 0; /* the lines that fit whole */
    for (uint64_t i = 0; i < capacity; i++)
      if (want[i] == '\n') whole = i + 1;
    if (memcmp(chars, want, whole) != 0) failures++;
    for (uint64_t i = whole; i < capacity; i++) failures += chars[i] != '#';
    free(chars);
  }
  if (!failures) printf("sam records: names and header of 4 records at every capacity: as expected\n");
  free(offsets);
  free(fv.headers);
  free(fv.records);
}

int main(void) {
  checkHand(1);
  checkHand(0);
  checkThreads();
  checkHeader();
  return failures ? 1 : 0;
}
