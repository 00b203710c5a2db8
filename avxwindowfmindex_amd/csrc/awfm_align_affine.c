/*
 * awfm_align_affine.c -- awfmAlignChainsAffine (include/awfm_gpu.h, "affine alignment"): the banded local alignment with affine
 * gap costs of every read against the record its chosen slot names, with soft clipping and the edit script.  The host twin of
 * awfmGpuAlignChainsAffine and its checker: a read at a time, the classification of the slot and the rows of the recurrence from
 * awfm_band.h (awfmClassifySlot, awfmAffineRows: three rows of at most 64 cells, shared with awfm_score_affine.c) with a trace
 * byte per cell in an n x width table, then the walk back through the three states.  awfmAlignChainsMatrix and
 * awfmAlignChainsEndBonus are the same call with the diagonal's score from a matrix, and with a bonus for a reached read end.
 * Exact and readable rather than fast.  The reference has no analogue (it stops at positions: ref src/AwFmParallelSearch.c:315-365).
 */
#include <stdlib.h>
#include <string.h>

#include "awfm_band.h"

enum { AWFM_OP_I = 1, AWFM_OP_D = 2, AWFM_OP_S = 4, AWFM_OP_EQ = 7, AWFM_OP_X = 8 };
enum { AWFM_STATE_H, AWFM_STATE_F, AWFM_STATE_E };

struct awfmAffineCtx {
  const struct AwFmVerifyInputs *in;
  const struct AwFmAffineOutputs *out;
  const uint32_t *chosen;
  const uint8_t *text;
  const uint64_t *ends;
  uint64_t length, numRecords;
  uint32_t slots, pad, drift, maxOps;
  struct awfmAffineCosts costs;
  int failed;
  uint64_t unaligned[64], truncated[64]; /* per thread of the loop */
};

struct awfmAffineAlignment {
  uint32_t score, distance, readBegin, readEnd, numOps;
  uint64_t textBegin, textEnd;
};

/* the runs come last to first */
struct awfmAffineRuns {
  uint32_t *ops;
  uint32_t maxOps, numOps, run, op;
};

static void awfmAffineFlush(struct awfmAffineRuns *s) {
  if (!s->run) return;
  if (s->ops && s->numOps < s->maxOps) s->ops[s->numOps] = s->run << 4 | s->op;
  s->numOps++;
  s->run = 0;
}

static void awfmAffineEmit(struct awfmAffineRuns *s, uint32_t op, uint32_t count) {
  if (!count) return;
  if (s->run && s->op != op) awfmAffineFlush(s);
  s->op = op;
  s->run += count;
}

/* R[0 .. n) against the record T[0 .. L) inside the diagonals [lo, hi] (hi - lo + 1 <= 64, anywhere relative to the record); the
 * runs go to ops[0 .. numOps) when numOps <= maxOps.  *table holds n x width trace bytes and grows as the thread meets longer
 * reads. */
static int awfmAffineRead(const struct awfmAffineCtx *c, const uint8_t *R, int64_t n, const uint8_t *T, int64_t L, int64_t lo, int64_t hi,
                          uint8_t **table, size_t *tableBytes, uint32_t *ops, struct awfmAffineAlignment *a) {
  const int64_t width = hi - lo + 1;
  memset(a, 0, sizeof *a);
  if (awfmAffineNoCell(n, L, lo, hi)) return 1;
  if ((size_t)(n * width) > *tableBytes) {
    free(*table);
    *tableBytes = (size_t)(n * width);
    *table = malloc(*tableBytes);
    if (!*table) {
      *tableBytes = 0;
      return 0;
    }
  }
  uint8_t *trace = *table;
  const struct awfmAffineEnd end = awfmAffineRows(&c->costs, R, n, T, L, lo, hi, trace);
  if (end.score == 0) return 1;
  a->score = (uint32_t)end.score;
  a->readEnd = (uint32_t)end.i;
  a->textEnd = (uint64_t)(end.i + lo + end.k);
  /* the walk meets the runs last to first: they are written in that order and turned round */
  struct awfmAffineRuns runs = {ops, c->maxOps, 0, 0, 0};
  awfmAffineEmit(&runs, AWFM_OP_S, (uint32_t)(n - end.i));
  int64_t i = end.i, k = end.k;
  int state = AWFM_STATE_H;
  uint32_t distance = 0;
  while (i > 0) {
    const uint8_t code = trace[(i - 1) * width + k];
    if (state == AWFM_STATE_H) {
      const uint8_t source = code & 7u;
      if (source == AWFM_SRC_STOP) break;
      if (source == AWFM_SRC_EQ || source == AWFM_SRC_X) {
        awfmAffineEmit(&runs, source == AWFM_SRC_X ? AWFM_OP_X : AWFM_OP_EQ, 1);
        distance += source == AWFM_SRC_X;
        i--;
        continue;
      }
      state = source == AWFM_SRC_F ? AWFM_STATE_F : AWFM_STATE_E;
    }
    distance++;
    if (state == AWFM_STATE_F) {
      awfmAffineEmit(&runs, AWFM_OP_I, 1);
      state = code & AWFM_TRACE_F_OPENS ? AWFM_STATE_H : AWFM_STATE_F;
      i--;
      k++;
    } else {
      awfmAffineEmit(&runs, AWFM_OP_D, 1);
      state = code & AWFM_TRACE_E_OPENS ? AWFM_STATE_H : AWFM_STATE_E;
      k--;
    }
  }
  awfmAffineEmit(&runs, AWFM_OP_S, (uint32_t)i);
  awfmAffineFlush(&runs);
  a->distance = distance;
  a->readBegin = (uint32_t)i;
  a->textBegin = (uint64_t)(i + lo + k);
  a->numOps = runs.numOps;
  if (ops && runs.numOps <= c->maxOps)
    for (uint32_t q = 0; q < runs.numOps / 2u; q++) {
      const uint32_t other = ops[runs.numOps - 1u - q];
      ops[runs.numOps - 1u - q] = ops[q];
      ops[q] = other;
    }
  return 1;
}

/* the status of read r, or its score (then < AWFM_VERIFY_TOO_LONG) with the alignment in *a */
static uint32_t awfmAffineOne(struct awfmAffineCtx *c, uint64_t r, uint8_t **table, size_t *tableBytes, struct awfmAffineAlignment *a) {
  const struct AwFmVerifyInputs *in = c->in;
  const uint32_t j = c->chosen[r];
  if (j == AWFM_CHAINS_NO_SLOT) return AWFM_VERIFY_NONE;
  if (j >= c->slots) return AWFM_VERIFY_MALFORMED;
  const uint64_t readBegin = in->readOffsets[r], readEnd = in->readOffsets[r + 1], n = readEnd - readBegin;
  struct awfmSlotBand b;
  const uint32_t status = awfmClassifySlot(in, c->ends, c->numRecords, c->length, c->drift, r * c->slots + j, n,
                                           readBegin <= readEnd && readEnd <= in->numReadChars, &b);
  if (status != AWFM_SLOT_HAS_BAND) return status;
  if (n > AWFM_ALIGN_MAX_LENGTH) return AWFM_VERIFY_TOO_LONG;
  const __int128 lo = (b.bD < b.eD ? b.bD : b.eD) - (__int128)c->pad, hi = (b.bD > b.eD ? b.bD : b.eD) + (__int128)c->pad;
  uint32_t *ops = c->out->ops ? c->out->ops + r * c->maxOps : NULL;
  if (!awfmAffineRead(c, in->readChars + readBegin, (int64_t)n, c->text + b.S, b.L, (int64_t)lo, (int64_t)hi, table, tableBytes, ops, a)) {
    c->failed = 1;
    return AWFM_VERIFY_NONE;
  }
  return a->score;
}

static void awfmAffineRange(void *p, uint64_t begin, uint64_t end, unsigned tid) {
  struct awfmAffineCtx *c = p;
  uint8_t *table = NULL;
  size_t tableBytes = 0;
  uint64_t unaligned = 0, truncated = 0;
  for (uint64_t r = begin; r < end; r++) {
    struct awfmAffineAlignment a;
    memset(&a, 0, sizeof a);
    const uint32_t value = awfmAffineOne(c, r, &table, &tableBytes, &a);
    if (value >= AWFM_VERIFY_TOO_LONG) {
      memset(&a, 0, sizeof a);
      if (value != AWFM_VERIFY_NONE) unaligned++;
    } else if (a.numOps > c->maxOps) {
      truncated++;
    }
    if (c->out->scores) c->out->scores[r] = value;
    if (c->out->editDistances) c->out->editDistances[r] = a.distance;
    if (c->out->readBegins) c->out->readBegins[r] = a.readBegin;
    if (c->out->readEnds) c->out->readEnds[r] = a.readEnd;
    if (c->out->textBegins) c->out->textBegins[r] = a.textBegin;
    if (c->out->textEnds) c->out->textEnds[r] = a.textEnd;
    if (c->out->numOps) c->out->numOps[r] = a.numOps;
  }
  free(table);
  c->unaligned[tid & 63u] += unaligned;
  c->truncated[tid & 63u] += truncated;
}

/* the call behind the entry points; scoring or matrix is given, the other is NULL; endBonus: 0 but for "end bonus" */
static enum AwFmReturnCode awfmAlignChainsScored(const struct AwFmVerifyInputs *in, const uint32_t *slots, uint64_t numReads,
                                                 uint32_t maxCandidates, uint32_t bandPad, uint32_t maxDrift,
                                                 const struct AwFmAlignScoring *scoring, const struct AwFmMatrixScoring *matrix,
                                                 uint32_t endBonus, uint32_t maxOps, const uint8_t *text, uint64_t length, const uint64_t *sequenceEnds,
                                                 uint64_t numRecords, enum AwFmAlphabetType alphabet, const struct AwFmAffineOutputs *out,
                                                 unsigned threads) {
  if (numReads == 0) return AwFmSuccess;
  const enum AwFmReturnCode rc = awfmBandCheckArguments(in, out && slots && (scoring || matrix), text, length, sequenceEnds, numRecords,
                                                        numReads, maxCandidates, bandPad, maxDrift);
  if (rc != AwFmSuccess) return rc;
  if (maxOps < 1 || maxOps > AWFM_ALIGN_MAX_OPS) return AwFmIllegalPositionError;
  if (!(matrix ? awfmMatrixScoringOk(matrix) : awfmScoringOk(scoring)) || endBonus > AWFM_END_BONUS_MAX) return AwFmIllegalPositionError;
  struct awfmAffineCtx ctx;
  memset(&ctx, 0, sizeof ctx);
  ctx.in = in;
  ctx.out = out;
  ctx.chosen = slots;
  ctx.text = text;
  ctx.ends = sequenceEnds;
  ctx.length = length;
  ctx.numRecords = numRecords;
  ctx.slots = maxCandidates;
  ctx.pad = bandPad;
  ctx.drift = maxDrift;
  ctx.maxOps = maxOps;
  ctx.costs = matrix ? awfmEndBonusCostsOf(matrix, endBonus, alphabet) : awfmAffineCostsOf(scoring, alphabet);
  awfmParallelFor(threads ? threads : 1, numReads, awfmAffineRange, &ctx);
  if (ctx.failed) return AwFmAllocationFailure;
  uint64_t unaligned = 0, truncated = 0;
  for (unsigned t = 0; t < 64; t++) {
    unaligned += ctx.unaligned[t];
    truncated += ctx.truncated[t];
  }
  if (out->numUnaligned) *out->numUnaligned += unaligned;
  if (out->numTruncated) *out->numTruncated += truncated;
  return AwFmSuccess;
}

enum AwFmReturnCode awfmAlignChainsAffine(const struct AwFmVerifyInputs *in, const uint32_t *slots, uint64_t numReads,
                                          uint32_t maxCandidates, uint32_t bandPad, uint32_t maxDrift,
                                          const struct AwFmAlignScoring *scoring, uint32_t maxOps, const uint8_t *text, uint64_t length,
                                          const uint64_t *sequenceEnds, uint64_t numRecords, enum AwFmAlphabetType alphabet,
                                          const struct AwFmAffineOutputs *out, unsigned threads) {
  return awfmAlignChainsScored(in, slots, numReads, maxCandidates, bandPad, maxDrift, scoring, NULL, 0, maxOps, text, length, sequenceEnds,
                               numRecords, alphabet, out, threads);
}

/* "substitution matrices" (include/awfm_gpu.h): the same call with s from the matrix */
enum AwFmReturnCode awfmAlignChainsMatrix(const struct AwFmVerifyInputs *in, const uint32_t *slots, uint64_t numReads,
                                          uint32_t maxCandidates, uint32_t bandPad, uint32_t maxDrift,
                                          const struct AwFmMatrixScoring *scoring, uint32_t maxOps, const uint8_t *text, uint64_t length,
                                          const uint64_t *sequenceEnds, uint64_t numRecords, enum AwFmAlphabetType alphabet,
                                          const struct AwFmAffineOutputs *out, unsigned threads) {
  return awfmAlignChainsScored(in, slots, numReads, maxCandidates, bandPad, maxDrift, NULL, scoring, 0, maxOps, text, length, sequenceEnds,
                               numRecords, alphabet, out, threads);
}

/* "end bonus" (include/awfm_gpu.h): the matrix call with B for a read end that is reached */
enum AwFmReturnCode awfmAlignChainsEndBonus(const struct AwFmVerifyInputs *in, const uint32_t *slots, uint64_t numReads,
                                            uint32_t maxCandidates, uint32_t bandPad, uint32_t maxDrift,
                                            const struct AwFmMatrixScoring *scoring, uint32_t endBonus, uint32_t maxOps, const uint8_t *text,
                                            uint64_t length, const uint64_t *sequenceEnds, uint64_t numRecords, enum AwFmAlphabetType alphabet,
                                            const struct AwFmAffineOutputs *out, unsigned threads) {
  return awfmAlignChainsScored(in, slots, numReads, maxCandidates, bandPad, maxDrift, NULL, scoring, endBonus, maxOps, text, length,
                               sequenceEnds, numRecords, alphabet, out, threads);
}
