/*
 * end_bonus_sanitize.c -- awfmScoreChainsEndBonus (csrc/awfm_score_affine.c) and awfmAlignChainsEndBonus
 * (csrc/awfm_align_affine.c) under AddressSanitizer and UBSan, as a stand-alone program.  The two twins get 2^13 random reads --
 * enough for the thread pool to cut the batch, a sixth of them cut from a record's first or last characters so that bands leave
 * the record and rows 0 and n lose their cells -- with every array in a heap block of exactly its size, under a matrix over the
 * full int8 range with B = 5 and B = 255, once on 1 thread and once on 16, whose outputs must be equal; with B = 0 they must
 * give what the matrix calls give, with B = 5 under the uniform matrix some read must reach an end it did not reach before, and
 * B = 256 is refused before anything is read.  Exit status 0: all of that held.
 *
 *   cc -std=gnu11 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude -Iavxwindowfmindex_amd/csrc \
 *      scripts/end_bonus_sanitize.c avxwindowfmindex_amd/csrc/awfm_matrix.c avxwindowfmindex_amd/csrc/awfm_score_affine.c \
 *      avxwindowfmindex_amd/csrc/awfm_align_affine.c avxwindowfmindex_amd/csrc/awfm_letters.c avxwindowfmindex_amd/csrc/awfm_threads.c \
 *      -pthread -static-libasan -static-libubsan -o end_bonus_sanitize && ./end_bonus_sanitize
 *
 * (tests/test_end_bonus_sanitizer.py does exactly that.)
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "AwFmIndex.h"
#include "awfm_gpu.h"

enum { READS = 1 << 13, SLOTS = 3, MAX_OPS = 6, TEXT = 1 << 14, RECORDS = 5, PAD = 3, DRIFT = 4 };

static int failures;

static void *exact(const void *from, size_t bytes) { /* a heap block of exactly `bytes` bytes */
  void *p = malloc(bytes ? bytes : 1);
  if (!p) abort();
  if (from && bytes) memcpy(p, from, bytes);
  return p;
}

static void expect(int ok, const char *what) {
  if (!ok) {
    fprintf(stderr, "FAILED: %s\n", what);
    failures++;
  }
}

static uint64_t lcgState = 2024;
static uint32_t lcg(uint32_t below) {
  lcgState = lcgState * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(lcgState >> 33) % below;
}

struct Batch {
  struct AwFmVerifyInputs in;
  uint8_t *text;
  uint64_t *ends;
  uint32_t *chosen;
};

struct Result {
  uint32_t *scores, *distances, *readBegins, *readEnds, *numOps, *ops, *slotScores, *slotReadEnds, *bestSlots, *bestScores, *secondSlots, *secondScores;
  uint64_t *textBegins, *textEnds, *slotTextEnds, counters[4];
  uint8_t *qualities;
};

static struct Batch makeBatch(void) {
  static const uint8_t letters[] = "acgtACGTnN$\0*u";
  struct Batch b;
  memset(&b, 0, sizeof b);
  b.text = exact(NULL, TEXT);
  for (uint64_t i = 0; i < TEXT; i++) b.text[i] = letters[lcg(lcg(8) ? 4 : sizeof letters - 1)];
  b.ends = exact(NULL, RECORDS * 8);
  for (uint64_t s = 0; s < RECORDS; s++) b.ends[s] = (s + 1) * (TEXT / RECORDS) - 1;
  const uint64_t recordLength = TEXT / RECORDS - 1;
  uint64_t *offsets = exact(NULL, (READS + 1) * 8);
  uint32_t *lengths = exact(NULL, READS * 4);
  offsets[0] = 0;
  for (uint64_t r = 0; r < READS; r++) {
    lengths[r] = r % 97 == 0 ? 0 : 1 + lcg(90);
    offsets[r + 1] = offsets[r] + lengths[r];
  }
  uint8_t *chars = exact(NULL, offsets[READS]);
  uint32_t *sequences = exact(NULL, READS * SLOTS * 4), *anchors = exact(NULL, READS * SLOTS * 4), *begins = exact(NULL, READS * SLOTS * 4),
           *endsOfChains = exact(NULL, READS * SLOTS * 4);
  int64_t *beginDiagonals = exact(NULL, READS * SLOTS * 8), *endDiagonals = exact(NULL, READS * SLOTS * 8);
  b.chosen = exact(NULL, READS * 4);
  for (uint64_t r = 0; r < READS; r++) {
    const uint32_t n = lengths[r], s = lcg(RECORDS);
    /* the read is cut from its record near its first or last characters now and then, so that bands leave the record */
    const uint64_t room = recordLength > n ? recordLength - n : 0, at = lcg(6) == 0 ? (lcg(2) ? 0 : room) : lcg((uint32_t)room + 1);
    const uint64_t S = s ? b.ends[s - 1] + 1 : 0;
    for (uint32_t i = 0; i < n; i++) chars[offsets[r] + i] = lcg(10) ? b.text[S + at + i] : letters[lcg(sizeof letters - 1)];
    b.chosen[r] = lcg(50) == 0 ? 0xFFFFFFFFu : lcg(SLOTS + (lcg(40) == 0));
    for (uint32_t j = 0; j < SLOTS; j++) {
      const uint64_t k = r * SLOTS + j;
      const uint32_t roll = lcg(20);
      sequences[k] = roll == 0 ? 0xFFFFFFFFu : roll == 1 ? RECORDS : j ? lcg(RECORDS) : s;
      anchors[k] = roll == 2 ? 0 : 1;
      begins[k] = n ? lcg(n) : 0;
      endsOfChains[k] = roll == 3 ? n + 1 : begins[k] + (n > begins[k] ? lcg(n - begins[k] + 1) : 0);
      beginDiagonals[k] = roll == 4 ? -(int64_t)begins[k] - 1 : (int64_t)at + (j ? (int64_t)lcg(9) - 4 : 0);
      endDiagonals[k] = beginDiagonals[k] + (roll == 5 ? DRIFT + 1 : (int64_t)lcg(2 * DRIFT + 1) - DRIFT);
      if (roll > 5 && (int64_t)endsOfChains[k] + endDiagonals[k] > (int64_t)recordLength) endDiagonals[k] = (int64_t)recordLength - endsOfChains[k];
    }
  }
  free(lengths);
  b.in.readChars = chars;
  b.in.numReadChars = offsets[READS];
  b.in.readOffsets = offsets;
  b.in.sequences = sequences;
  b.in.chainAnchors = anchors;
  b.in.chainReadBegins = begins;
  b.in.chainReadEnds = endsOfChains;
  b.in.chainBeginDiagonals = beginDiagonals;
  b.in.chainEndDiagonals = endDiagonals;
  return b;
}

static struct Result makeResult(void) {
  struct Result r;
  memset(&r, 0, sizeof r);
  r.scores = exact(NULL, READS * 4);
  r.distances = exact(NULL, READS * 4);
  r.readBegins = exact(NULL, READS * 4);
  r.readEnds = exact(NULL, READS * 4);
  r.numOps = exact(NULL, READS * 4);
  r.ops = calloc((size_t)READS * MAX_OPS, 4);
  r.textBegins = exact(NULL, READS * 8);
  r.textEnds = exact(NULL, READS * 8);
  r.slotScores = exact(NULL, READS * SLOTS * 4);
  r.slotReadEnds = exact(NULL, READS * SLOTS * 4);
  r.slotTextEnds = exact(NULL, READS * SLOTS * 8);
  r.bestSlots = exact(NULL, READS * 4);
  r.bestScores = exact(NULL, READS * 4);
  r.secondSlots = exact(NULL, READS * 4);
  r.secondScores = exact(NULL, READS * 4);
  r.qualities = exact(NULL, READS);
  return r;
}

static void freeResult(struct Result *r) {
  void *blocks[] = {r->scores,     r->distances,    r->readBegins,   r->readEnds,  r->numOps,     r->ops,         r->textBegins,   r->textEnds,
                    r->slotScores, r->slotReadEnds, r->slotTextEnds, r->bestSlots, r->bestScores, r->secondSlots, r->secondScores, r->qualities};
  for (size_t i = 0; i < sizeof blocks / sizeof blocks[0]; i++) free(blocks[i]);
}

/* both twins on `threads` threads; bonus == NO_BONUS: the matrix calls */
enum { NO_BONUS = 0xFFFFFFFFu };
static struct Result run(const struct Batch *b, const struct AwFmMatrixScoring *matrix, uint32_t bonus, unsigned threads) {
  struct Result r = makeResult();
  const struct AwFmAffineOutputs aligned = {r.scores,  r.distances, r.readBegins, r.readEnds,      r.textBegins,
                                            r.textEnds, r.numOps,    r.ops,        &r.counters[0], &r.counters[1]};
  const struct AwFmSlotScoreOutputs scored = {r.slotScores,  r.slotReadEnds, r.slotTextEnds, r.bestSlots,    r.bestScores,
                                              r.secondSlots, r.secondScores, r.qualities,    &r.counters[2], &r.counters[3]};
  enum AwFmReturnCode rcAlign, rcScore;
  if (bonus == NO_BONUS) {
    rcAlign = awfmAlignChainsMatrix(&b->in, b->chosen, READS, SLOTS, PAD, DRIFT, matrix, MAX_OPS, b->text, TEXT, b->ends, RECORDS, AwFmAlphabetDna, &aligned, threads);
    rcScore = awfmScoreChainsMatrix(&b->in, READS, SLOTS, PAD, DRIFT, matrix, 2, 60, b->text, TEXT, b->ends, RECORDS, AwFmAlphabetDna, &scored, threads);
  } else {
    rcAlign = awfmAlignChainsEndBonus(&b->in, b->chosen, READS, SLOTS, PAD, DRIFT, matrix, bonus, MAX_OPS, b->text, TEXT, b->ends, RECORDS, AwFmAlphabetDna, &aligned, threads);
    rcScore = awfmScoreChainsEndBonus(&b->in, READS, SLOTS, PAD, DRIFT, matrix, bonus, 2, 60, b->text, TEXT, b->ends, RECORDS, AwFmAlphabetDna, &scored, threads);
  }
  expect(rcAlign == AwFmSuccess && rcScore == AwFmSuccess, "the calls succeed");
  return r;
}

static int sameResults(const struct Result *a, const struct Result *b) {
  int same = memcmp(a->counters, b->counters, sizeof a->counters) == 0;
  same &= !memcmp(a->scores, b->scores, READS * 4) && !memcmp(a->distances, b->distances, READS * 4) && !memcmp(a->readBegins, b->readBegins, READS * 4);
  same &= !memcmp(a->readEnds, b->readEnds, READS * 4) && !memcmp(a->numOps, b->numOps, READS * 4) && !memcmp(a->textBegins, b->textBegins, READS * 8);
  same &= !memcmp(a->textEnds, b->textEnds, READS * 8) && !memcmp(a->slotScores, b->slotScores, READS * SLOTS * 4);
  same &= !memcmp(a->slotReadEnds, b->slotReadEnds, READS * SLOTS * 4) && !memcmp(a->slotTextEnds, b->slotTextEnds, READS * SLOTS * 8);
  same &= !memcmp(a->bestSlots, b->bestSlots, READS * 4) && !memcmp(a->bestScores, b->bestScores, READS * 4) && !memcmp(a->secondSlots, b->secondSlots, READS * 4);
  same &= !memcmp(a->secondScores, b->secondScores, READS * 4) && !memcmp(a->qualities, b->qualities, READS);
  for (uint64_t r = 0; r < READS && same; r++) /* (the row of a truncated read is unspecified) */
    if (a->scores[r] < AWFM_VERIFY_TOO_LONG && a->numOps[r] <= MAX_OPS) same &= !memcmp(a->ops + r * MAX_OPS, b->ops + r * MAX_OPS, a->numOps[r] * 4);
  return same;
}

int main(void) {
  const struct Batch b = makeBatch();
  struct AwFmMatrixScoring *wild = exact(NULL, sizeof *wild); /* the struct itself in a block of its size */
  for (uint32_t i = 0; i < AWFM_MATRIX_CLASSES * AWFM_MATRIX_CLASSES; i++) wild->substitution[i] = (int8_t)((int)lcg(256) - 128);
  for (uint32_t i = 0; i < 4; i++) wild->substitution[i * AWFM_MATRIX_CLASSES + i] = (int8_t)(60 + lcg(68));
  wild->gapOpen = 6;
  wild->gapExtend = 1;
  const uint32_t bonuses[] = {5, 255};
  for (uint32_t k = 0; k < 2; k++) {
    struct Result one = run(&b, wild, bonuses[k], 1), sixteen = run(&b, wild, bonuses[k], 16);
    uint64_t aligned = 0;
    for (uint64_t r = 0; r < READS; r++) aligned += one.scores[r] > 0 && one.scores[r] < AWFM_VERIFY_TOO_LONG;
    expect(aligned > READS / 2 && one.counters[0] > 100 && one.counters[2] > 100 && one.counters[3] > READS / 2, "the batch has aligned reads and statuses");
    expect(sameResults(&one, &sixteen), "1 and 16 threads agree under the full-range matrix");
    printf("full-range matrix, B = %u: %" PRIu64 " reads aligned, 1 and 16 threads agree\n", bonuses[k], aligned);
    freeResult(&one);
    freeResult(&sixteen);
  }
  const struct AwFmAlignScoring scoring = {1, 4, 6, 1};
  struct AwFmMatrixScoring *uniform = exact(NULL, sizeof *uniform);
  expect(awfmMatrixScoringUniform(AwFmAlphabetDna, &scoring, uniform) == AwFmSuccess, "the uniform matrix");
  struct Result plain = run(&b, uniform, NO_BONUS, 16), zero = run(&b, uniform, 0, 16), five = run(&b, uniform, 5, 1);
  expect(sameResults(&plain, &zero), "B = 0 gives what the matrix calls give");
  printf("B = 0: equal to the matrix calls\n");
  uint64_t reached = 0;
  for (uint64_t r = 0; r < READS; r++)
    if (plain.scores[r] > 0 && plain.scores[r] < AWFM_VERIFY_TOO_LONG && five.scores[r] < AWFM_VERIFY_TOO_LONG)
      reached += (plain.readBegins[r] > 0 && five.readBegins[r] == 0) || (five.readEnds[r] > plain.readEnds[r]);
  expect(reached > 100, "B = 5 lets reads reach ends they did not reach");
  printf("B = 5: %" PRIu64 " reads reach an end they did not reach without it\n", reached);
  struct AwFmAffineOutputs none;
  struct AwFmSlotScoreOutputs noScores;
  memset(&none, 0, sizeof none);
  memset(&noScores, 0, sizeof noScores);
  expect(awfmAlignChainsEndBonus(&b.in, b.chosen, READS, SLOTS, PAD, DRIFT, uniform, 256, MAX_OPS, b.text, TEXT, b.ends, RECORDS, AwFmAlphabetDna, &none, 1) ==
             AwFmIllegalPositionError,
         "B = 256 is refused by the alignment call");
  expect(awfmScoreChainsEndBonus(&b.in, READS, SLOTS, PAD, DRIFT, uniform, 256, 2, 60, b.text, TEXT, b.ends, RECORDS, AwFmAlphabetDna, &noScores, 1) ==
             AwFmIllegalPositionError,
         "B = 256 is refused by the scoring call");
  freeResult(&plain);
  freeResult(&zero);
  freeResult(&five);
  free(wild);
  free(uniform);
  free((void *)b.in.readChars);
  free((void *)b.in.readOffsets);
  free((void *)b.in.sequences);
  free((void *)b.in.chainAnchors);
  free((void *)b.in.chainReadBegins);
  free((void *)b.in.chainReadEnds);
  free((void *)b.in.chainBeginDiagonals);
  free((void *)b.in.chainEndDiagonals);
  free(b.text);
  free(b.ends);
  free(b.chosen);
  if (failures) return 1;
  printf("end bonus: clean\n");
  return 0;
}
