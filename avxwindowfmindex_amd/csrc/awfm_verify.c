/*
 * awfm_verify.c -- awfmTextWindows and awfmVerifyChains (include/awfm_gpu.h, "chain verification"): batched recall of the indexed
 * text, and the banded global edit distance of every chain against the text it names.  The host twins of awfmGpuTextWindows and
 * awfmGpuVerifyChains and their checkers: a read at a time, two rows of at most 64 cells, the recurrence as the header states it.
 * Nothing here is clever.  ref src/AwFmFile.c (awFmReadSequenceFromFile: one segment per call); the reference has no analogue of
 * the verification (it stops at positions: ref src/AwFmParallelSearch.c:315-365).
 */
#include <string.h>

#include "awfm_gpu.h"
#include "awfm_internal.h"

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
  uint32_t slots, pad, drift, proper;
  int amino;
  uint64_t unverified[64]; /* per thread of the loop */
};

/* 0 when both characters map to the same proper letter */
static uint32_t awfmVerifySub(const struct awfmVerifyCtx *c, uint8_t a, uint8_t b) {
  const uint8_t x = c->amino ? awfmAminoAsciiToIndex(a) : awfmNucAsciiToIndex(a);
  const uint8_t y = c->amino ? awfmAminoAsciiToIndex(b) : awfmNucAsciiToIndex(b);
  return x == y && x < c->proper ? 0u : 1u;
}

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
        if (j >= 1 && prev[k] != AWFM_VERIFY_INF) best = prev[k] + awfmVerifySub(c, R[i - 1], T[j - 1]);
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
  const uint32_t s = in->sequences[at];
  if (s == AWFM_CANDIDATES_NONE || in->chainAnchors[at] == 0) return AWFM_VERIFY_NONE;
  const uint64_t readBegin = in->readOffsets[r], readEnd = in->readOffsets[r + 1];
  if (readBegin > readEnd || readEnd > in->numReadChars) return AWFM_VERIFY_MALFORMED;
  const uint64_t rb = in->chainReadBegins[at], re = in->chainReadEnds[at];
  if (rb > re || re > readEnd - readBegin) return AWFM_VERIFY_MALFORMED;
  if (s >= (c->numRecords ? c->numRecords : 1u)) return AWFM_VERIFY_MALFORMED;
  const uint64_t S = c->numRecords && s ? c->ends[s - 1] + 1u : 0u, E = c->numRecords ? c->ends[s] : c->length;
  if (c->numRecords && s && S == 0) return AWFM_VERIFY_MALFORMED; /* (an end of 2^64 - 1) */
  if (E < S || E > c->length) return AWFM_VERIFY_MALFORMED;
  const __int128 tb = (__int128)rb + in->chainBeginDiagonals[at], te = (__int128)re + in->chainEndDiagonals[at];
  if (tb < 0 || tb > te || te > (__int128)(E - S)) return AWFM_VERIFY_MALFORMED;
  const int64_t n = (int64_t)(re - rb), m = (int64_t)(te - tb), delta = m - n; /* m <= length < 2^63, n < 2^32 */
  if (delta > (int64_t)c->drift || delta < -(int64_t)c->drift) return AWFM_VERIFY_TOO_WIDE;
  if (n > (int64_t)AWFM_VERIFY_MAX_LENGTH) return AWFM_VERIFY_TOO_LONG;
  const int64_t lo = (delta < 0 ? delta : 0) - (int64_t)c->pad, hi = (delta > 0 ? delta : 0) + (int64_t)c->pad;
  return awfmBandedDistance(c, in->readChars + readBegin + rb, n, c->text + S + (uint64_t)tb, m, lo, hi);
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
  if (!in || !out || !in->readOffsets || !in->sequences || !in->chainAnchors || !in->chainReadBegins || !in->chainReadEnds ||
      !in->chainBeginDiagonals || !in->chainEndDiagonals)
    return AwFmNullPtrError;
  if ((!in->readChars && in->numReadChars != 0) || (!text && length != 0) || (!sequenceEnds && numRecords != 0)) return AwFmNullPtrError;
  if (numReads >= (1ull << 32) || maxCandidates < 1 || maxCandidates > AWFM_CANDIDATES_MAX_SLOTS) return AwFmIllegalPositionError;
  if ((uint64_t)maxDrift + 2ull * bandPad + 1ull > AWFM_VERIFY_MAX_BAND) return AwFmIllegalPositionError;
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
  ctx.proper = ctx.amino ? 20u : 4u;
  awfmParallelFor(threads ? threads : 1, numReads, awfmVerifyRange, &ctx);
  uint64_t unverified = 0;
  for (unsigned t = 0; t < 64; t++) unverified += ctx.unverified[t];
  if (out->numUnverified) *out->numUnverified += unverified;
  return AwFmSuccess;
}
