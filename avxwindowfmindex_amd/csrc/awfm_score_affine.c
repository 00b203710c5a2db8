/*
 * awfm_score_affine.c -- awfmScoreChainsAffine (include/awfm_gpu.h, "slot scores and mapping quality"): the banded local affine
 * score and end cell of EVERY slot of every read, and per read the best slot, the runner-up and a mapping quality.  The host twin
 * of awfmGpuScoreChainsAffine and its checker: a read at a time, the recurrence of "affine alignment" as the header states it with
 * three rows of at most 64 cells, no trace table and no walk; then the per-read rules, written plainly over the read's C results.
 * A slot gets what awfmAlignChainsAffine (awfm_align_affine.c) puts into scores, readEnds and textEnds when slots[r] names it:
 * tests/test_score_chains.py holds the two files to that.  Exact and readable rather than fast.  The reference has no analogue
 * (it stops at positions: ref src/AwFmParallelSearch.c:315-365).
 */
#include <stdlib.h>
#include <string.h>

#include "awfm_gpu.h"
#include "awfm_internal.h"

#define AWFM_SCORE_NEG INT32_MIN /* minus infinity: awfmScoreMinus keeps it what it is */

struct awfmScoreCtx {
  const struct AwFmVerifyInputs *in;
  const struct AwFmSlotScoreOutputs *out;
  const uint8_t *text;
  const uint64_t *ends;
  uint64_t length, numRecords;
  uint32_t slots, pad, drift, proper, minScore, cap;
  int32_t match, mismatch, open, extend;
  int amino;
  uint64_t unscored[64], mapped[64]; /* per thread of the loop */
};

struct awfmSlotScore {
  uint32_t value, readEnd, sequence; /* value: a score or a status */
  uint64_t textEnd;
};

static uint32_t awfmScoreSub(const struct awfmScoreCtx *c, uint8_t a, uint8_t b) {
  const uint8_t x = c->amino ? awfmAminoAsciiToIndex(a) : awfmNucAsciiToIndex(a);
  const uint8_t y = c->amino ? awfmAminoAsciiToIndex(b) : awfmNucAsciiToIndex(b);
  return x == y && x < c->proper ? 0u : 1u;
}

static int32_t awfmScoreMinus(int32_t value, int32_t cost) { return value == AWFM_SCORE_NEG ? AWFM_SCORE_NEG : value - cost; }
static int32_t awfmScoreMax(int32_t a, int32_t b) { return a > b ? a : b; }

/* R[0 .. n) against the record T[0 .. L) inside the diagonals [lo, hi] (hi - lo + 1 <= 64, anywhere relative to the record): the
 * largest H over existing cells with i >= 1, then the smallest i, then the smallest t; a score of 0 comes with zeros */
static void awfmScoreRead(const struct awfmScoreCtx *c, const uint8_t *R, int64_t n, const uint8_t *T, int64_t L, int64_t lo, int64_t hi,
                          struct awfmSlotScore *a) {
  int32_t rowsH[2][AWFM_VERIFY_MAX_BAND], rowsF[2][AWFM_VERIFY_MAX_BAND], E[AWFM_VERIFY_MAX_BAND];
  const int64_t width = hi - lo + 1;
  a->value = 0;
  a->readEnd = 0;
  a->textEnd = 0;
  if (n == 0 || n + hi < 0 || lo + 1 > L) return; /* no existing cell with i >= 1: nothing is read */
  int32_t *prevH = rowsH[0], *curH = rowsH[1], *prevF = rowsF[0], *curF = rowsF[1];
  const int32_t open = c->open + c->extend, extend = c->extend;
  for (int64_t k = 0; k < width; k++) { /* row 0 */
    const int64_t t = lo + k;
    prevH[k] = t >= 0 && t <= L ? 0 : AWFM_SCORE_NEG;
    prevF[k] = AWFM_SCORE_NEG;
  }
  int32_t best = 0;
  int64_t bestI = 0, bestK = 0;
  for (int64_t i = 1; i <= n; i++) {
    for (int64_t k = 0; k < width; k++) {
      const int64_t t = i + lo + k;
      curH[k] = curF[k] = E[k] = AWFM_SCORE_NEG;
      if (t < 0 || t > L) continue;
      /* (i-1, t-1) lies on the same diagonal, (i-1, t) on the next one up, (i, t-1) on the one below */
      const int32_t M = t >= 1 ? awfmScoreMinus(prevH[k], awfmScoreSub(c, R[i - 1], T[t - 1]) ? c->mismatch : -c->match) : AWFM_SCORE_NEG;
      const int32_t F = awfmScoreMax(awfmScoreMinus(k + 1 < width ? prevH[k + 1] : AWFM_SCORE_NEG, open),
                                     awfmScoreMinus(k + 1 < width ? prevF[k + 1] : AWFM_SCORE_NEG, extend));
      const int32_t e = awfmScoreMax(awfmScoreMinus(k >= 1 ? curH[k - 1] : AWFM_SCORE_NEG, open),
                                     awfmScoreMinus(k >= 1 ? E[k - 1] : AWFM_SCORE_NEG, extend));
      const int32_t H = awfmScoreMax(awfmScoreMax(0, M), awfmScoreMax(F, e));
      curH[k] = H;
      curF[k] = F;
      E[k] = e;
      if (H > best) { /* rows in ascending order, then columns: the smallest i, then the smallest t of the largest H */
        best = H;
        bestI = i;
        bestK = k;
      }
    }
    int32_t *swap = prevH;
    prevH = curH;
    curH = swap;
    swap = prevF;
    prevF = curF;
    curF = swap;
  }
  if (best == 0) return;
  a->value = (uint32_t)best;
  a->readEnd = (uint32_t)bestI;
  a->textEnd = (uint64_t)(bestI + lo + bestK);
}

/* slot j of read r: the order of the checks is awfmAlignChainsAffine's with slots[r] = j < C */
static void awfmScoreSlot(const struct awfmScoreCtx *c, uint64_t r, uint32_t j, struct awfmSlotScore *a) {
  const struct AwFmVerifyInputs *in = c->in;
  const uint64_t at = r * c->slots + j;
  const uint32_t s = in->sequences[at];
  a->readEnd = 0;
  a->textEnd = 0;
  a->sequence = s;
  a->value = AWFM_VERIFY_MALFORMED;
  if (s == AWFM_CANDIDATES_NONE || in->chainAnchors[at] == 0) {
    a->value = AWFM_VERIFY_NONE;
    return;
  }
  const uint64_t readBegin = in->readOffsets[r], readEnd = in->readOffsets[r + 1];
  if (readBegin > readEnd || readEnd > in->numReadChars) return;
  const uint64_t rb = in->chainReadBegins[at], re = in->chainReadEnds[at], n = readEnd - readBegin;
  if (rb > re || re > n) return;
  if (s >= (c->numRecords ? c->numRecords : 1u)) return;
  const uint64_t S = c->numRecords && s ? c->ends[s - 1] + 1u : 0u, E = c->numRecords ? c->ends[s] : c->length;
  if (c->numRecords && s && S == 0) return; /* (an end of 2^64 - 1) */
  if (E < S || E > c->length) return;
  const int64_t bD = in->chainBeginDiagonals[at], eD = in->chainEndDiagonals[at];
  const __int128 tb = (__int128)rb + bD, te = (__int128)re + eD;
  if (tb < 0 || tb > te || te > (__int128)(E - S)) return;
  /* 0 <= tb <= te <= L < 2^63 and rb, re < 2^32: both diagonals lie in (-2^32, 2^63) and their difference is exact */
  const __int128 delta = (__int128)eD - bD;
  if (delta > (__int128)c->drift || delta < -(__int128)c->drift) {
    a->value = AWFM_VERIFY_TOO_WIDE;
    return;
  }
  if (n > AWFM_ALIGN_MAX_LENGTH) {
    a->value = AWFM_VERIFY_TOO_LONG;
    return;
  }
  const __int128 lo = (bD < eD ? bD : eD) - (__int128)c->pad, hi = (bD > eD ? bD : eD) + (__int128)c->pad;
  awfmScoreRead(c, in->readChars + readBegin, (int64_t)n, c->text + S, (int64_t)(E - S), (int64_t)lo, (int64_t)hi, a);
}

static void awfmScoreRange(void *p, uint64_t begin, uint64_t end, unsigned tid) {
  struct awfmScoreCtx *c = p;
  const struct AwFmSlotScoreOutputs *out = c->out;
  const uint32_t C = c->slots, floor = c->minScore > 1u ? c->minScore : 1u;
  uint64_t unscored = 0, mapped = 0;
  for (uint64_t r = begin; r < end; r++) {
    struct awfmSlotScore slot[AWFM_CANDIDATES_MAX_SLOTS];
    for (uint32_t j = 0; j < C; j++) {
      awfmScoreSlot(c, r, j, &slot[j]);
      const uint32_t v = slot[j].value;
      if (v >= AWFM_VERIFY_TOO_LONG && v != AWFM_VERIFY_NONE) unscored++;
      if (out->slotScores) out->slotScores[r * C + j] = v;
      if (out->slotReadEnds) out->slotReadEnds[r * C + j] = slot[j].readEnd;
      if (out->slotTextEnds) out->slotTextEnds[r * C + j] = slot[j].textEnd;
    }
    /* 1, 2: the counting slot of the largest score, ties to the lowest slot */
    uint32_t best = AWFM_CHAINS_NO_SLOT, bestScore = 0, second = AWFM_CHAINS_NO_SLOT, secondScore = 0;
    for (uint32_t j = 0; j < C; j++) {
      const uint32_t v = slot[j].value;
      if (v < AWFM_VERIFY_TOO_LONG && v >= floor && v > bestScore) {
        best = j;
        bestScore = v;
      }
    }
    /* 3, 4: of the other counting slots, those that are not the best one's alignment again */
    for (uint32_t j = 0; j < C && best != AWFM_CHAINS_NO_SLOT; j++) {
      const uint32_t v = slot[j].value;
      if (j == best || v >= AWFM_VERIFY_TOO_LONG || v < floor) continue;
      if (slot[j].sequence == slot[best].sequence && slot[j].readEnd == slot[best].readEnd && slot[j].textEnd == slot[best].textEnd) continue;
      if (v > secondScore) {
        second = j;
        secondScore = v;
      }
    }
    /* 5: exact in 32 bits, best < 2^24 and cap <= 254 */
    const uint32_t quality = best == AWFM_CHAINS_NO_SLOT ? 0u : c->cap * (bestScore - secondScore) / bestScore;
    mapped += best != AWFM_CHAINS_NO_SLOT;
    if (out->bestSlots) out->bestSlots[r] = best;
    if (out->bestScores) out->bestScores[r] = bestScore;
    if (out->secondSlots) out->secondSlots[r] = second;
    if (out->secondScores) out->secondScores[r] = secondScore;
    if (out->mappingQualities) out->mappingQualities[r] = (uint8_t)quality;
  }
  c->unscored[tid & 63u] += unscored;
  c->mapped[tid & 63u] += mapped;
}

enum AwFmReturnCode awfmScoreChainsAffine(const struct AwFmVerifyInputs *in, uint64_t numReads, uint32_t maxCandidates, uint32_t bandPad,
                                          uint32_t maxDrift, const struct AwFmAlignScoring *scoring, uint32_t minScore, uint32_t mapqCap,
                                          const uint8_t *text, uint64_t length, const uint64_t *sequenceEnds, uint64_t numRecords,
                                          enum AwFmAlphabetType alphabet, const struct AwFmSlotScoreOutputs *out, unsigned threads) {
  if (numReads == 0) return AwFmSuccess;
  if (!in || !out || !scoring || !in->readOffsets || !in->sequences || !in->chainAnchors || !in->chainReadBegins || !in->chainReadEnds ||
      !in->chainBeginDiagonals || !in->chainEndDiagonals)
    return AwFmNullPtrError;
  if ((!in->readChars && in->numReadChars != 0) || (!text && length != 0) || (!sequenceEnds && numRecords != 0)) return AwFmNullPtrError;
  if (numReads >= (1ull << 32) || maxCandidates < 1 || maxCandidates > AWFM_CANDIDATES_MAX_SLOTS) return AwFmIllegalPositionError;
  if ((uint64_t)maxDrift + 2ull * bandPad + 1ull > AWFM_VERIFY_MAX_BAND) return AwFmIllegalPositionError;
  if (mapqCap > AWFM_SCORE_MAX_MAPQ) return AwFmIllegalPositionError;
  if (scoring->match < 1 || scoring->match > 255 || scoring->mismatch > 255 || scoring->gapOpen > 255 || scoring->gapExtend < 1 ||
      scoring->gapExtend > 255)
    return AwFmIllegalPositionError;
  struct awfmScoreCtx ctx;
  memset(&ctx, 0, sizeof ctx);
  ctx.in = in;
  ctx.out = out;
  ctx.text = text;
  ctx.ends = sequenceEnds;
  ctx.length = length;
  ctx.numRecords = numRecords;
  ctx.slots = maxCandidates;
  ctx.pad = bandPad;
  ctx.drift = maxDrift;
  ctx.minScore = minScore;
  ctx.cap = mapqCap;
  ctx.match = (int32_t)scoring->match;
  ctx.mismatch = (int32_t)scoring->mismatch;
  ctx.open = (int32_t)scoring->gapOpen;
  ctx.extend = (int32_t)scoring->gapExtend;
  ctx.amino = alphabet == AwFmAlphabetAmino;
  ctx.proper = ctx.amino ? 20u : 4u;
  awfmParallelFor(threads ? threads : 1, numReads, awfmScoreRange, &ctx);
  uint64_t unscored = 0, mapped = 0;
  for (unsigned t = 0; t < 64; t++) {
    unscored += ctx.unscored[t];
    mapped += ctx.mapped[t];
  }
  if (out->numUnscored) *out->numUnscored += unscored;
  if (out->numMapped) *out->numMapped += mapped;
  return AwFmSuccess;
}
