/*
 * awfm_verify.c -- awfmTextWindows and awfmVerifyChains (include/awfm_gpu.h, "chain verification"): batched recall of the indexed
 * text, and the banded global edit distance of every chain against the text it names.  The host twins of awfmGpuTextWindows and
 * awfmGpuVerifyChains and their checkers: a read at a time, two rows of at most 64 cells, the recurrence as the header states it.
 * Nothing here is clever; the classification of a slot, the letter comparison and the argument checks are awfm_band.h's, shared
 * with the other twins of the read path.  ref src/AwFmFile.c (awFmReadSequenceFromFile: one segment per call); the reference has no analogue of
 * the verification (it stops at positions: ref src/AwFmParallelSearch.c:315-365).
 */
#include <string.h>

#include "awfm_band.h"

#define AWFM_VERIFY_INF 0x3FFFFFFFu /* a cell outside the matrix */

struct awfmWindowsCtx {
  const uint8_t *text;
  uint64_t length;
  const uint64_t *positions;
  uint32_t before, after;
  uint8_t *out;
};

static void awfmWindowsRange(void *p, uint64_t begin, uint64_t end, unsigned tid) {
  const struct awfmWindowsCtx *c = p;
  (void)tid;
  const uint64_t width = (uint64_t)c->before + c->after;
  for (uint64_t i = begin; i < end; i++) {
    uint8_t *window = c->out + i * width;
    const uint64_t at = c->positions[i];
    memset(window, 0, width);
    if (at >= c->length) continue;
    /* [at - before, at + after) cut to [0, length): at < length < 2^63, so neither sum wraps */
    const uint64_t from = at >= c->before ? at - c->before : 0, to = at + c->after < c->length ? at + c->after : c->length;
    if (to > from) memcpy(window + (from + c->before - at), c->text + from, to - from);
  }
}

enum AwFmReturnCode awfmTextWindows(const uint8_t *text, uint64_t length, const uint64_t *positions, uint64_t numPositions, uint32_t before,
                                    uint32_t after, uint8_t *out, unsigned threads) {
  const uint64_t width = (uint64_t)before + after;
  if (width < 1 || width > 4096) return AwFmIllegalPositionError;
  if (numPositions == 0) return AwFmSuccess;
  if (!positions || !out || (!text && length != 0)) return AwFmNullPtrError;
  struct awfmWindowsCtx ctx = {text, length, positions, before, after, out};
  awfmParallelFor(threads ? threads : 1, numPositions, awfmWindowsRange, &ctx);
  return AwFmSuccess;
}

struct awfmVerifyCtx {
  const struct AwFmVerifyInputs *in;
  const struct AwFmVerifyOutputs *out;
  const uint8_t *text;
  const uint64_t *ends;
  uint64_t length, numRecords;
  uint32_t slots, pad, drift;
  int amino;
  uint64_t unverified[64]; /* per thread of the loop */
};

/* H(n, m) of R[0 .. n) against T[0 .. m) inside the band [lo, hi] of diagonals j - i (hi - lo + 1 <= 64) */
static uint32_t awfmBandedDistance(const struct awfmVerifyCtx *c, const uint8_t *R, int64_t n, const uint8_t *T, int64_t m, int64_t lo,
                                   int64_t hi) {
  uint32_t rows[2][AWFM_VERIFY_MAX_BAND];
  const int64_t width = hi - lo + 1;
  uint32_t *prev = rows[0], *cur = rows[1];
  for (int64_t k = 0; k < width; k++) { /* row 0: H(0, j) = j along the row, for the j the band holds */
    const int64_t j = lo + k;
    prev[k] = j >= 0 && j <= m ? (uint32_t)j : AWFM_VERIFY_INF;
  }
  for (int64_t i = 1; i <= n; i++) {
    for (int64_t k = 0; k < width; k++) {
      const int64_t j = i + lo + k;
      uint32_t best = AWFM_VERIFY_INF;
      if (j >= 0 && j <= m) {
        /* (i-1, j-1) lies on the same diagonal, (i-1, j) on the next one up, (i, j-1) on the one below */
        if (j >= 1 && prev[k] != AWFM_VERIFY_INF) best = prev[k] + awfmBandSub(c->amino, R[i - 1], T[j - 1]);
        if (k + 1 < width && prev[k + 1] != AWFM_VERIFY_INF && prev[k + 1] + 1u < best) best = prev[k + 1] + 1u;
        if (k >= 1 && cur[k - 1] != AWFM_VERIFY_INF && cur[k - 1] + 1u < best) best = cur[k - 1] + 1u;
      }
      cur[k] = best;
    }
    uint32_t *swap = prev;
    prev = cur;
    cur = swap;
  }
  return prev[m - n - lo];
}

static uint32_t awfmVerifySlot(const struct awfmVerifyCtx *c, uint64_t r, uint64_t at) {
  const struct AwFmVerifyInputs *in = c->in;
  const uint64_t readBegin = in->readOffsets[r], readEnd = in->readOffsets[r + 1];
  struct awfmSlotBand b;
  const uint32_t status = awfmClassifySlot(in, c->ends, c->numRecords, c->length, c->drift, at, readEnd - readBegin,
                                           readBegin <= readEnd && readEnd <= in->numReadChars, &b);
  if (status != AWFM_SLOT_HAS_BAND) return status;
  /* the span alone, and the band relative to it: diagonal 0 is the span's first cell, the drift its last one's */
  const int64_t n = (int64_t)(b.re - b.rb), delta = b.eD - b.bD, m = n + delta;
  if (n > (int64_t)AWFM_VERIFY_MAX_LENGTH) return AWFM_VERIFY_TOO_LONG;
  const int64_t lo = (delta < 0 ? delta : 0) - (int64_t)c->pad, hi = (delta > 0 ? delta : 0) + (int64_t)c->pad;
  return awfmBandedDistance(c, in->readChars + readBegin + b.rb, n, c->text + b.S + (uint64_t)b.tb, m, lo, hi);
}

static void awfmVerifyRange(void *p, uint64_t begin, uint64_t end, unsigned tid) {
  struct awfmVerifyCtx *c = p;
  uint64_t unverified = 0;
  for (uint64_t r = begin; r < end; r++) {
    uint32_t bestSlot = AWFM_CHAINS_NO_SLOT, bestDistance = 0;
    for (uint32_t j = 0; j < c->slots; j++) {
      const uint64_t at = r * c->slots + j;
      const uint32_t distance = awfmVerifySlot(c, r, at);
      if (distance >= AWFM_VERIFY_TOO_LONG) {
        if (distance != AWFM_VERIFY_NONE) unverified++;
      } else if (bestSlot == AWFM_CHAINS_NO_SLOT || distance < bestDistance) { /* (ties: the lowest slot) */
        bestSlot = j;
        bestDistance = distance;
      }
      if (c->out->editDistances) c->out->editDistances[at] = distance;
    }
    if (c->out->bestSlots) c->out->bestSlots[r] = bestSlot;
  }
  c->unverified[tid & 63u] += unverified;
}

enum AwFmReturnCode awfmVerifyChains(const struct AwFmVerifyInputs *in, uint64_t numReads, uint32_t maxCandidates, uint32_t bandPad,
                                     uint32_t maxDrift, const uint8_t *text, uint64_t length, const uint64_t *sequenceEnds,
                                     uint64_t numRecords, enum AwFmAlphabetType alphabet, const struct AwFmVerifyOutputs *out,
                                     unsigned threads) {
  if (numReads == 0) return AwFmSuccess;
  const enum AwFmReturnCode rc = awfmBandCheckArguments(in, out != NULL, text, length, sequenceEnds, numRecords, numReads, maxCandidates, bandPad, maxDrift);
  if (rc != AwFmSuccess) return rc;
  struct awfmVerifyCtx ctx;
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
  ctx.amino = alphabet == AwFmAlphabetAmino;
  awfmParallelFor(threads ? threads : 1, numReads, awfmVerifyRange, &ctx);
  uint64_t unverified = 0;
  for (unsigned t = 0; t < 64; t++) unverified += ctx.unverified[t];
  if (out->numUnverified) *out->numUnverified += unverified;
  return AwFmSuccess;
}
