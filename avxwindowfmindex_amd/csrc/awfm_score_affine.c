/*
 * awfm_score_affine.c -- awfmScoreChainsAffine (include/awfm_gpu.h, "slot scores and mapping quality"): the banded local affine
 * score and end cell of EVERY slot of every read, and per read the best slot, the runner-up and a mapping quality.  The host twin
 * of awfmGpuScoreChainsAffine and its checker: a read at a time, the classification of a slot and the rows of "affine alignment"
 * from awfm_band.h, without a trace table and without the walk; then the per-read rules, written plainly over the read's C results.
 * A slot gets what awfmAlignChainsAffine (awfm_align_affine.c) puts into scores, readEnds and textEnds when slots[r] names it:
 * both files call the same rows, and tests/test_score_chains.py checks it.  awfmScoreChainsMatrix and awfmScoreChainsEndBonus are
 * the same call with the diagonal's score from a matrix, and with a bonus for a reached read end.  Exact and readable rather than
 * fast.  The reference has no analogue
 * (it stops at positions: ref src/AwFmParallelSearch.c:315-365).
 */
#include <stdlib.h>
#include <string.h>

#include "awfm_band.h"

struct awfmScoreCtx {
  const struct AwFmVerifyInputs *in;
  const struct AwFmSlotScoreOutputs *out;
  const uint8_t *text;
  const uint64_t *ends;
  uint64_t length, numRecords;
  uint32_t slots, pad, drift, minScore, cap;
  struct awfmAffineCosts costs;
  uint64_t unscored[64], mapped[64]; /* per thread of the loop */
};

struct awfmSlotScore {
  uint32_t value, readEnd, sequence; /* value: a score or a status */
  uint64_t textEnd;
};

/* slot j of read r: a status, or the score and end cell of the rows of "affine alignment"; a score of 0 comes with zeros */
static void awfmScoreSlot(const struct awfmScoreCtx *c, uint64_t r, uint32_t j, struct awfmSlotScore *a) {
  const struct AwFmVerifyInputs *in = c->in;
  const uint64_t at = r * c->slots + j;
  const uint64_t readBegin = in->readOffsets[r], readEnd = in->readOffsets[r + 1], n = readEnd - readBegin;
  struct awfmSlotBand b;
  a->readEnd = 0;
  a->textEnd = 0;
  a->sequence = in->sequences[at];
  a->value = awfmClassifySlot(in, c->ends, c->numRecords, c->length, c->drift, at, n, readBegin <= readEnd && readEnd <= in->numReadChars, &b);
  if (a->value != AWFM_SLOT_HAS_BAND) return;
  if (n > AWFM_ALIGN_MAX_LENGTH) {
    a->value = AWFM_VERIFY_TOO_LONG;
    return;
  }
  const __int128 lo = (b.bD < b.eD ? b.bD : b.eD) - (__int128)c->pad, hi = (b.bD > b.eD ? b.bD : b.eD) + (__int128)c->pad;
  a->value = 0;
  if (awfmAffineNoCell((int64_t)n, b.L, (int64_t)lo, (int64_t)hi)) return;
  const struct awfmAffineEnd end = awfmAffineRows(&c->costs, in->readChars + readBegin, (int64_t)n, c->text + b.S, b.L, (int64_t)lo, (int64_t)hi, NULL);
  if (end.score == 0) return;
  a->value = (uint32_t)end.score;
  a->readEnd = (uint32_t)end.i;
  a->textEnd = (uint64_t)(end.i + (int64_t)lo + end.k);
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

/* the call behind the entry points; scoring or matrix is given, the other is NULL; endBonus: 0 but for "end bonus" */
static enum AwFmReturnCode awfmScoreChainsScored(const struct AwFmVerifyInputs *in, uint64_t numReads, uint32_t maxCandidates, uint32_t bandPad,
                                                 uint32_t maxDrift, const struct AwFmAlignScoring *scoring,
                                                 const struct AwFmMatrixScoring *matrix, uint32_t endBonus, uint32_t minScore, uint32_t mapqCap,
                                                 const uint8_t *text, uint64_t length, const uint64_t *sequenceEnds, uint64_t numRecords,
                                                 enum AwFmAlphabetType alphabet, const struct AwFmSlotScoreOutputs *out, unsigned threads) {
  if (numReads == 0) return AwFmSuccess;
  const enum AwFmReturnCode rc = awfmBandCheckArguments(in, out && (scoring || matrix), text, length, sequenceEnds, numRecords, numReads,
                                                        maxCandidates, bandPad, maxDrift);
  if (rc != AwFmSuccess) return rc;
  if (mapqCap > AWFM_SCORE_MAX_MAPQ) return AwFmIllegalPositionError;
  if (!(matrix ? awfmMatrixScoringOk(matrix) : awfmScoringOk(scoring)) || endBonus > AWFM_END_BONUS_MAX) return AwFmIllegalPositionError;
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
  ctx.costs = matrix ? awfmEndBonusCostsOf(matrix, endBonus, alphabet) : awfmAffineCostsOf(scoring, alphabet);
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

enum AwFmReturnCode awfmScoreChainsAffine(const struct AwFmVerifyInputs *in, uint64_t numReads, uint32_t maxCandidates, uint32_t bandPad,
                                          uint32_t maxDrift, const struct AwFmAlignScoring *scoring, uint32_t minScore, uint32_t mapqCap,
                                          const uint8_t *text, uint64_t length, const uint64_t *sequenceEnds, uint64_t numRecords,
                                          enum AwFmAlphabetType alphabet, const struct AwFmSlotScoreOutputs *out, unsigned threads) {
  return awfmScoreChainsScored(in, numReads, maxCandidates, bandPad, maxDrift, scoring, NULL, 0, minScore, mapqCap, text, length, sequenceEnds,
                               numRecords, alphabet, out, threads);
}

/* "substitution matrices" (include/awfm_gpu.h): the same call with s from the matrix */
enum AwFmReturnCode awfmScoreChainsMatrix(const struct AwFmVerifyInputs *in, uint64_t numReads, uint32_t maxCandidates, uint32_t bandPad,
                                          uint32_t maxDrift, const struct AwFmMatrixScoring *scoring, uint32_t minScore, uint32_t mapqCap,
                                          const uint8_t *text, uint64_t length, const uint64_t *sequenceEnds, uint64_t numRecords,
                                          enum AwFmAlphabetType alphabet, const struct AwFmSlotScoreOutputs *out, unsigned threads) {
  return awfmScoreChainsScored(in, numReads, maxCandidates, bandPad, maxDrift, NULL, scoring, 0, minScore, mapqCap, text, length, sequenceEnds,
                               numRecords, alphabet, out, threads);
}

/* "end bonus" (include/awfm_gpu.h): the matrix call with B for a read end that is reached */
enum AwFmReturnCode awfmScoreChainsEndBonus(const struct AwFmVerifyInputs *in, uint64_t numReads, uint32_t maxCandidates, uint32_t bandPad,
                                            uint32_t maxDrift, const struct AwFmMatrixScoring *scoring, uint32_t endBonus, uint32_t minScore,
                                            uint32_t mapqCap, const uint8_t *text, uint64_t length, const uint64_t *sequenceEnds,
                                            uint64_t numRecords, enum AwFmAlphabetType alphabet, const struct AwFmSlotScoreOutputs *out,
                                            unsigned threads) {
  return awfmScoreChainsScored(in, numReads, maxCandidates, bandPad, maxDrift, NULL, scoring, endBonus, minScore, mapqCap, text, length,
                               sequenceEnds, numRecords, alphabet, out, threads);
}
