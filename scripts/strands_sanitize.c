/*
 * strands_sanitize.c -- awfmChooseStrands and awfmOrientReads (csrc/awfm_strands.c) under AddressSanitizer and UBSan, as a
 * stand-alone program: pairs written out by hand -- a proper pair from either strand of the fragment, bests on one strand, one
 * mate placed, none placed, a malformed read, windows whose bounds go below 0 --, paired and unpaired, with every array in a heap
 * block of exactly its size, so that a read or a write one byte outside any of them stops the program; every output NULL; then
 * 2^12 random reads at 1, 5 and 16 slots a row on 1 and on 16 threads, whose outputs must be equal; and the orienting gather on
 * exact blocks: every read length 0 to 70, both strands, qualities reversed, malformed reads, a capacity that cuts the last read.
 * Exit status 0: every value is the expected one.
 *
 *   cc -std=gnu11 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude -Iavxwindowfmindex_amd/csrc \
 *      scripts/strands_sanitize.c avxwindowfmindex_amd/csrc/awfm_strands.c avxwindowfmindex_amd/csrc/awfm_threads.c \
 *      -pthread -static-libasan -static-libubsan -o strands_sanitize && ./strands_sanitize
 *
 * (tests/test_strands_sanitizer.py does exactly that.)
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "AwFmIndex.h"
#include "awfm_gpu.h"
#include "awfm_internal.h"

static int failures;

#define CHECK(condition, ...)       \
  do {                              \
    if (!(condition)) {             \
      failures++;                   \
      printf("FAILED: " __VA_ARGS__); \
      printf("\n");                 \
    }                               \
  } while (0)

static void *exact(const void *from, size_t bytes) { /* a heap block of exactly `bytes` bytes */
  void *p = malloc(bytes ? bytes : 1);
  if (from && bytes) memcpy(p, from, bytes);
  else if (bytes) memset(p, 0xA5, bytes);
  return p;
}

enum { C_HAND = 2, PAIRS = 7, READS = 2 * PAIRS, ROWS = 2 * READS };
#define NA AWFM_VERIFY_NONE
#define NS AWFM_CHAINS_NO_SLOT
#define NW AWFM_CANDIDATES_NONE

/* a slot whose start is S: readEnd 100, textEnd S + 100 */
struct Slot {
  uint32_t score, sequence;
  int64_t start;
};
static const struct Slot unused = {NA, NW, -100};

/* per pair: the first slot of rows F(m1), V(m1), F(m2), V(m2) (the second slot of every row is unused) */
static const struct Slot hand[PAIRS][4] = {
    {{50, 0, 1000}, {NA, NW, -100}, {NA, NW, -100}, {40, 0, 1200}}, /* proper, m1 forward: T = 1200 + 100 - 1000 */
    {{NA, NW, -100}, {50, 0, 1200}, {40, 0, 1000}, {NA, NW, -100}}, /* proper, m1 reverse */
    {{50, 0, 1000}, {NA, NW, -100}, {50, 0, 1200}, {NA, NW, -100}}, /* bests on strand 0: discordant, 100 - 17 */
    {{NA, NW, -100}, {60, 3, -60}, {NA, NW, -100}, {NA, NW, -100}}, /* only m1, on strand 1, S = -60: m2's window [0, 0) on F */
    {{NA, NW, -100}, {NA, NW, -100}, {NA, NW, -100}, {NA, NW, -100}}, /* none placed */
    {{70, 0, 1000}, {70, 0, 1000}, {50, 0, 1000}, {NA, NW, -100}},   /* m1 malformed (reverse row of 90): m2 alone */
    {{50, 0, 1000}, {50, 0, 3000}, {NA, NW, -100}, {NA, NW, -100}},  /* a tie between strands: strand 0, quality 0 */
};
static const uint8_t wantProper[PAIRS] = {1, 1, 0, 0, 0, 0, 0};
static const uint32_t wantPairScores[PAIRS] = {90, 90, 83, 60, 0, 50, 50};
static const int64_t wantLengths[PAIRS] = {300, 300, 0, 0, 0, 0, 0};
static const uint8_t wantStrands[READS] = {0, 1, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0};
static const uint32_t wantSlots[READS] = {0, 0, 0, 0, 0, 0, 0, NS, NS, NS, NS, 0, 0, NS};
static const uint8_t wantQualities[READS] = {60, 60, 60, 60, 60, 60, 60, 0, 0, 0, 0, 60, 0, 0};
/* the windows: (row, sequence, begin, end); every other row has none */
static const struct {
  uint32_t row, sequence;
  uint64_t begin, end;
} wantWindows[] = {
    {READS + 4, 0, 1250, 1750}, {READS + 5, 0, 1050, 1550}, /* pair 2: both on the V rows */
    {7, 3, 0, 0},                                           /* pair 3: F(m2), E = 40 */
    {READS + 10, 0, 1050, 1550},                            /* pair 5: V(m1) from m2's best on strand 0 */
    {READS + 13, 0, 1050, 1550},                            /* pair 6: V(m2) */
};

static void handWritten(void) {
  uint64_t offsets[ROWS + 1];
  uint32_t sequences[ROWS * C_HAND], scores[ROWS * C_HAND], readEnds[ROWS * C_HAND];
  uint64_t textEnds[ROWS * C_HAND];
  offsets[0] = 7;
  for (unsigned row = 0; row < ROWS; row++) offsets[row + 1] = offsets[row] + (row == READS + 10 ? 90u : 100u);
  for (unsigned p = 0; p < PAIRS; p++)
    for (unsigned k = 0; k < 4; k++) {
      const unsigned row = (k & 1u) * READS + 2u * p + (k >> 1);
      const struct Slot both[C_HAND] = {hand[p][k], unused};
      for (unsigned j = 0; j < C_HAND; j++) {
        sequences[row * C_HAND + j] = both[j].sequence;
        scores[row * C_HAND + j] = both[j].score;
        readEnds[row * C_HAND + j] = both[j].score == NA ? 0u : 100u;
        textEnds[row * C_HAND + j] = both[j].score == NA ? 0u : (uint64_t)(both[j].start + 100);
      }
    }
  struct AwFmStrandInputs in = {exact(offsets, sizeof offsets), exact(sequences, sizeof sequences), exact(scores, sizeof scores),
                                exact(readEnds, sizeof readEnds), exact(textEnds, sizeof textEnds)};
  const struct AwFmPairParams params = {200, 500, 0, 17, 50, 60};
  for (uint32_t paired = 0; paired < 2; paired++) {
    uint64_t counters[4] = {1, 2, 3, 4};
    struct AwFmStrandOutputs out = {exact(NULL, READS),     exact(NULL, 4 * READS), exact(NULL, 4 * READS), exact(NULL, 4 * READS), exact(NULL, READS),
                                    exact(NULL, 2 * READS), exact(NULL, 4 * ROWS),  exact(NULL, 4 * ROWS),  exact(NULL, 8 * ROWS),  exact(NULL, 8 * ROWS),
                                    exact(NULL, PAIRS),     exact(NULL, 4 * PAIRS), exact(NULL, 4 * PAIRS), exact(NULL, 8 * PAIRS), exact(NULL, PAIRS),
                                    &counters[0],           &counters[1],           &counters[2],           &counters[3]};
    const enum AwFmReturnCode rc = awfmChooseStrands(&in, READS, C_HAND, paired ? AWFM_STRANDS_PAIRED : 0u, &params, &out, 3);
    CHECK(rc == AwFmSuccess, "awfmChooseStrands returned %d", (int)rc);
    CHECK(counters[3] == 4 + 1, "numMalformed %" PRIu64, counters[3]);
    if (paired) {
      CHECK(counters[0] == 1 + 3 && counters[1] == 2 + 2 && counters[2] == 3 + 5, "counters %" PRIu64 " %" PRIu64 " %" PRIu64, counters[0],
            counters[1], counters[2]);
      for (unsigned p = 0; p < PAIRS; p++) {
        CHECK(out.properPairs[p] == wantProper[p] && out.pairScores[p] == wantPairScores[p] && out.templateLengths[p] == wantLengths[p],
              "pair %u: %u %u %" PRId64, p, out.properPairs[p], out.pairScores[p], out.templateLengths[p]);
        CHECK(out.pairQualities[p] == (wantProper[p] ? 60 : 0) && out.pairSecondScores[p] == 0, "pair %u: quality %u second %u", p,
              out.pairQualities[p], out.pairSecondScores[p]);
      }
      for (unsigned r = 0; r < READS; r++) {
        CHECK(out.strands[r] == wantStrands[r] && out.strandSlots[r] == wantSlots[r] && out.baseFlags[r] == 0x10u * wantStrands[r],
              "read %u: strand %u slot %u flags %u", r, out.strands[r], out.strandSlots[r], out.baseFlags[r]);
        CHECK(out.mappingQualities[r] == wantQualities[r], "read %u: quality %u", r, out.mappingQualities[r]);
      }
      for (unsigned row = 0; row < ROWS; row++) {
        uint32_t sequence = NW;
        uint64_t begin = 0, end = 0;
        for (unsigned w = 0; w < sizeof wantWindows / sizeof wantWindows[0]; w++)
          if (wantWindows[w].row == row) sequence = wantWindows[w].sequence, begin = wantWindows[w].begin, end = wantWindows[w].end;
        CHECK(out.windowSequences[row] == sequence && out.windowBegins[row] == begin && out.windowEnds[row] == end,
              "row %u: window %u %" PRIu64 " %" PRIu64, row, out.windowSequences[row], out.windowBegins[row], out.windowEnds[row]);
        const unsigned r = row % READS;
        CHECK(out.rowSlots[row] == (wantSlots[r] != NS && wantStrands[r] == row / READS ? wantSlots[r] : NS), "row %u: slot %u", row, out.rowSlots[row]);
      }
    } else {
      CHECK(counters[0] == 1 + 3 && counters[1] == 2 && counters[2] == 3, "unpaired counters %" PRIu64 " %" PRIu64 " %" PRIu64, counters[0], counters[1],
            counters[2]);
      CHECK(out.strands[1] == 1 && out.strands[2] == 1 && out.strands[6] == 1 && out.strands[12] == 0, "unpaired strands");
      CHECK(out.bestScores[12] == 50 && out.secondScores[12] == 50 && out.mappingQualities[12] == 0 && out.mappingQualities[0] == 60, "unpaired scores");
      CHECK(out.bestScores[10] == 0 && out.strandSlots[10] == NS, "the malformed read is placed");
      for (unsigned row = 0; row < ROWS; row++) CHECK(out.windowSequences[row] == NW && out.windowEnds[row] == 0, "unpaired window at row %u", row);
      CHECK(out.properPairs[0] == 0xA5 && out.pairScores[PAIRS - 1] == 0xA5A5A5A5u, "unpaired wrote a pair array");
    }
    void *blocks[] = {out.strands,      out.strandSlots,  out.bestScores,       out.secondScores,    out.mappingQualities,
                      out.baseFlags,    out.rowSlots,     out.windowSequences,  out.windowBegins,    out.windowEnds,
                      out.properPairs,  out.pairScores,   out.pairSecondScores, out.templateLengths, out.pairQualities};
    for (unsigned i = 0; i < sizeof blocks / sizeof blocks[0]; i++) free(blocks[i]);
    const struct AwFmStrandOutputs nothing = {0};
    CHECK(awfmChooseStrands(&in, READS, C_HAND, paired, &params, &nothing, 2) == AwFmSuccess, "every output NULL");
  }
  printf("hand-written pairs, paired and unpaired: %s\n", failures ? "NOT as expected" : "as expected");
  free((void *)in.readOffsets);
  free((void *)in.sequences);
  free((void *)in.slotScores);
  free((void *)in.slotReadEnds);
  free((void *)in.slotTextEnds);
}

static uint64_t state = 88172645463325252ull;
static uint64_t next(void) {
  state ^= state << 13;
  state ^= state >> 7;
  state ^= state << 17;
  return state;
}

static void randomTables(void) {
  enum { R = 1 << 12 };
  const int before = failures;
  for (unsigned c = 0; c < 3; c++) {
    const uint32_t C = c == 0 ? 1u : c == 1 ? 5u : 16u;
    uint64_t *offsets = exact(NULL, 8 * (2 * R + 1));
    uint32_t *sequences = exact(NULL, 4ull * 2 * R * C), *scores = exact(NULL, 4ull * 2 * R * C), *readEnds = exact(NULL, 4ull * 2 * R * C);
    uint64_t *textEnds = exact(NULL, 8ull * 2 * R * C);
    offsets[0] = 0;
    for (unsigned row = 0; row < 2 * R; row++) {
      const unsigned r = row % R;
      uint64_t n = 50 + r % 100;
      if (row >= R && r % 97 == 3) n += 1; /* rows of two lengths */
      offsets[row + 1] = r % 89 == 5 && row < R ? offsets[row] - 1 : offsets[row] + n;
      for (unsigned j = 0; j < C; j++) {
        const uint64_t x = next();
        const unsigned at = row * C + j;
        scores[at] = x % 5 == 0 ? 0xFFFFFFFFu - (uint32_t)(x >> 8) % 4 : (uint32_t)(x >> 8) % 12;
        sequences[at] = (uint32_t)(x >> 16) % 2;
        readEnds[at] = (uint32_t)(x >> 20) % 150;
        textEnds[at] = (r / 2) * 1000 + (row >= R ? 190 : 0) + 10 * ((x >> 32) % 7) + readEnds[at];
        if (j && x % 7 == 1) scores[at] = scores[at - 1], sequences[at] = sequences[at - 1], readEnds[at] = readEnds[at - 1], textEnds[at] = textEnds[at - 1];
      }
    }
    const struct AwFmStrandInputs in = {offsets, sequences, scores, readEnds, textEnds};
    const struct AwFmPairParams params = {150, 500, 2, 3, 20, 254};
    for (uint32_t paired = 0; paired < 2; paired++) {
      struct AwFmStrandOutputs out[2];
      uint64_t counters[2][4];
      for (unsigned t = 0; t < 2; t++) {
        memset(counters[t], 0, sizeof counters[t]);
        out[t] = (struct AwFmStrandOutputs){exact(NULL, R),     exact(NULL, 4 * R),     exact(NULL, 4 * R),     exact(NULL, 4 * R),     exact(NULL, R),
                                            exact(NULL, 2 * R), exact(NULL, 8 * R),     exact(NULL, 8 * R),     exact(NULL, 16 * R),    exact(NULL, 16 * R),
                                            exact(NULL, R / 2), exact(NULL, 2 * R),     exact(NULL, 2 * R),     exact(NULL, 4 * R),     exact(NULL, R / 2),
                                            &counters[t][0],    &counters[t][1],        &counters[t][2],        &counters[t][3]};
        CHECK(awfmChooseStrands(&in, R, C, paired, &params, &out[t], t ? 16 : 1) == AwFmSuccess, "random tables: a refusal");
      }
      const size_t sizes[15] = {R, 4 * R, 4 * R, 4 * R, R, 2 * R, 8 * R, 8 * R, 16 * R, 16 * R, R / 2, 2 * R, 2 * R, 4 * R, R / 2};
      void **a = (void **)&out[0], **b = (void **)&out[1];
      for (unsigned i = 0; i < 15; i++) {
        CHECK(!memcmp(a[i], b[i], sizes[i]), "C = %u paired %u: output %u differs between 1 and 16 threads", C, paired, i);
        free(a[i]);
        free(b[i]);
      }
      CHECK(!memcmp(counters[0], counters[1], sizeof counters[0]), "C = %u: counters differ", C);
      CHECK(counters[0][3] > R / 100 && (!paired || (counters[0][1] > R / 64 && counters[0][2] > R / 64)) && counters[0][0] > R / 8,
            "C = %u paired %u: counters %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64, C, paired, counters[0][0], counters[0][1], counters[0][2],
            counters[0][3]);
    }
    free(offsets);
    free(sequences);
    free(scores);
    free(readEnds);
    free(textEnds);
  }
  if (failures == before) printf("random tables: 1 and 16 threads agree\n");
}

static void orient(void) {
  enum { R = 71, C = 3 };
  const int before = failures;
  uint64_t offsets[2 * R + 1], total = 0;
  offsets[0] = 5;
  for (unsigned row = 0; row < 2 * R; row++) offsets[row + 1] = offsets[row] + row % R; /* lengths 0 .. 70, twice */
  total = offsets[R] - offsets[0];
  const uint64_t numChars = offsets[2 * R];
  uint8_t *chars = exact(NULL, numChars), *qualities = exact(NULL, numChars), strands[R];
  for (uint64_t i = 0; i < numChars; i++) chars[i] = (uint8_t)next(), qualities[i] = (uint8_t)(33 + next() % 90);
  for (unsigned r = 0; r < R; r++) strands[r] = (uint8_t)(next() & 1u);
  strands[40] = 2; /* malformed: a strand above 1 */
  uint32_t *anchors = exact(NULL, 4 * 2 * R * C), *scores = exact(NULL, 4 * 2 * R * C);
  int64_t *diagonals = exact(NULL, 8 * 2 * R * C);
  for (unsigned i = 0; i < 2 * R * C; i++) anchors[i] = i, scores[i] = 7 * i, diagonals[i] = -(int64_t)i;
  for (unsigned cut = 0; cut < 2; cut++) { /* the whole capacity, then one that the last read does not fit */
    const uint64_t capacity = total - cut;
    struct AwFmOrientInputs in;
    struct AwFmOrientOutputs out;
    uint64_t malformed = 10;
    memset(&in, 0, sizeof in);
    memset(&out, 0, sizeof out);
    in.rows.readChars = chars;
    in.rows.numReadChars = numChars;
    in.rows.readOffsets = exact(offsets, sizeof offsets);
    in.rows.chainAnchors = anchors;
    in.rows.chainEndDiagonals = diagonals;
    in.slotScores = scores;
    in.qualities = qualities;
    in.strands = exact(strands, sizeof strands);
    out.readChars = exact(NULL, capacity);
    out.capacity = capacity;
    out.readOffsets = exact(NULL, 8 * (R + 1));
    out.qualities = exact(NULL, capacity);
    out.chainAnchors = exact(NULL, 4 * R * C);
    out.chainEndDiagonals = exact(NULL, 8 * R * C);
    out.slotScores = exact(NULL, 4 * R * C);
    out.numMalformed = &malformed;
    CHECK(awfmOrientReads(&in, R, C, &out, cut ? 16 : 1) == AwFmSuccess, "awfmOrientReads: a refusal");
    CHECK(malformed == 10 + 1 + cut, "orient: numMalformed %" PRIu64, malformed);
    for (unsigned r = 0; r < R; r++) {
      const uint64_t to = offsets[r] - offsets[0], n = r;
      const int good = r != 40 && !(cut && r == R - 1);
      CHECK(out.readOffsets[r] == to, "orient: readOffsets[%u]", r);
      for (uint64_t i = 0; i < n && to + i < capacity; i++) {
        const uint8_t wantChar = good ? chars[offsets[strands[r] ? R + r : r] + i] : 0xA5;
        const uint8_t wantQuality = good ? qualities[offsets[r] + (strands[r] ? n - 1 - i : i)] : 0xA5;
        CHECK(out.readChars[to + i] == wantChar && out.qualities[to + i] == wantQuality, "orient: byte %" PRIu64 " of read %u", i, r);
      }
      for (unsigned j = 0; j < C; j++) {
        const unsigned source = ((strands[r] == 1 ? R : 0) + r) * C + j;
        CHECK(out.chainAnchors[r * C + j] == (good ? anchors[source] : 0u) && out.slotScores[r * C + j] == (good ? scores[source] : AWFM_VERIFY_NONE) &&
                  out.chainEndDiagonals[r * C + j] == (good ? diagonals[source] : 0),
              "orient: columns of read %u", r);
      }
    }
    CHECK(out.readOffsets[R] == total, "orient: readOffsets[R]");
    free((void *)in.rows.readOffsets);
    free((void *)in.strands);
    free(out.readChars);
    free(out.readOffsets);
    free(out.qualities);
    free(out.chainAnchors);
    free(out.chainEndDiagonals);
    free(out.slotScores);
  }
  free(chars);
  free(qualities);
  free(anchors);
  free(scores);
  free(diagonals);
  if (failures == before) printf("orient on exact blocks: as expected\n");
}

int main(void) {
  handWritten();
  randomTables();
  orient();
  if (failures) printf("%d FAILED\n", failures);
  return failures ? 1 : 0;
}
