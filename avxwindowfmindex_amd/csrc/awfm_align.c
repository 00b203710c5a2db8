/*
 * awfm_align.c -- awfmAlignChains (include/awfm_gpu.h, "chain alignment"): the banded fitting alignment of every read against the
 * record its chosen slot names, with the edit script.  The host twin of awfmGpuAlignChains and its checker: a read at a time,
 * the recurrence as the header states it with a direction byte per cell in an n x band table, then the walk back.  The
 * classification of the slot, the letter comparison and the argument checks are awfm_band.h's.  Exact and readable rather than
 * fast.  The reference has no analogue (it stops at positions: ref src/AwFmParallelSearch.c:315-365).
 */
#include <stdlib.h>
#include <string.h>

#include "awfm_band.h"

#define AWFM_ALIGN_INF 0x3FFFFFFFu /* a cell that does not exist */
enum { AWFM_DIR_DIAGONAL = 0, AWFM_DIR_UP = 1, AWFM_DIR_LEFT = 2 };
enum { AWFM_OP_I = 1, AWFM_OP_D = 2, AWFM_OP_EQ = 7, AWFM_OP_X = 8 };

struct awfmAlignCtx {
  const struct AwFmVerifyInputs *in;
  const struct AwFmAlignOutputs *out;
  const uint32_t *chosen;
  const uint8_t *text;
  const uint64_t *ends;
  uint64_t length, numRecords;
  uint32_t slots, pad, drift, maxOps;
  int amino, failed;
  uint64_t unaligned[64], truncated[64]; /* per thread of the loop */
};

struct awfmAlignment {
  uint32_t distance, numOps;
  uint64_t textBegin, textEnd;
};

/* R[0 .. n) against the record T[0 .. L) inside the diagonals [lo, hi] (hi >= 0, lo + n <= L, hi - lo + 1 <= 64); the runs go to
 * ops[0 .. numOps) when numOps <= maxOps.  *table holds n x width direction bytes and grows as the thread meets longer reads. */
static int awfmAlignRead(const struct awfmAlignCtx *c, const uint8_t *R, int64_t n, const uint8_t *T, int64_t L, int64_t lo, int64_t hi,
                         uint8_t **table, size_t *tableBytes, uint32_t *ops, struct awfmAlignment *a) {
  uint32_t rows[2][AWFM_VERIFY_MAX_BAND];
  const int64_t width = hi - lo + 1;
  if ((size_t)(n * width) > *tableBytes) {
    free(*table);
    *tableBytes = (size_t)(n * width);
    *table = malloc(*tableBytes);
    if (!*table) {
      *tableBytes = 0;
      return 0;
    }
  }
  uint8_t *directions = *table;
  uint32_t *prev = rows[0], *cur = rows[1];
  for (int64_t k = 0; k < width; k++) { /* row 0: free in the text */
    const int64_t t = lo + k;
    prev[k] = t >= 0 && t <= L ? 0u : AWFM_ALIGN_INF;
  }
  for (int64_t i = 1; i <= n; i++) {
    for (int64_t k = 0; k < width; k++) {
      const int64_t t = i + lo + k;
      uint32_t best = AWFM_ALIGN_INF;
      uint8_t direction = AWFM_DIR_LEFT;
      if (t >= 0 && t <= L) {
        /* (i-1, t-1) lies on the same diagonal, (i-1, t) on the next one up, (i, t-1) on the one below */
        const uint32_t diagonal = t >= 1 && prev[k] != AWFM_ALIGN_INF ? prev[k] + awfmBandSub(c->amino, R[i - 1], T[t - 1]) : AWFM_ALIGN_INF;
        const uint32_t up = k + 1 < width && prev[k + 1] != AWFM_ALIGN_INF ? prev[k + 1] + 1u : AWFM_ALIGN_INF;
        const uint32_t left = k >= 1 && cur[k - 1] != AWFM_ALIGN_INF ? cur[k - 1] + 1u : AWFM_ALIGN_INF;
        best = diagonal < up ? diagonal : up;
        best = left < best ? left : best;
        direction = diagonal == best ? AWFM_DIR_DIAGONAL : up == best ? AWFM_DIR_UP : AWFM_DIR_LEFT;
      }
      cur[k] = best;
      directions[(i - 1) * width + k] = direction;
    }
    uint32_t *swap = prev;
    prev = cur;
    cur = swap;
  }
  int64_t k = -1;
  for (int64_t q = 0; q < width; q++) /* the smallest t of the smallest value */
    if (prev[q] != AWFM_ALIGN_INF && (k < 0 || prev[q] < prev[k])) k = q;
  if (k < 0) return 0; /* (never: the header's finiteness argument) */
  a->distance = prev[k];
  a->textEnd = (uint64_t)(n + lo + k);
  /* the walk meets the runs last to first: they are written in that order and turned round */
  uint32_t numOps = 0, run = 0, op = 0;
  int64_t i = n;
  while (i > 0) {
    const int64_t t = i + lo + k;
    const uint8_t direction = directions[(i - 1) * width + k];
    uint32_t now;
    if (direction == AWFM_DIR_DIAGONAL) {
      now = awfmBandSub(c->amino, R[i - 1], T[t - 1]) ? AWFM_OP_X : AWFM_OP_EQ;
      i--;
    } else if (direction == AWFM_DIR_UP) {
      now = AWFM_OP_I;
      i--;
      k++;
    } else {
      now = AWFM_OP_D;
      k--;
    }
    if (run && now != op) {
      if (ops && numOps < c->maxOps) ops[numOps] = run << 4 | op;
      numOps++;
      run = 0;
    }
    op = now;
    run++;
  }
  if (run) {
    if (ops && numOps < c->maxOps) ops[numOps] = run << 4 | op;
    numOps++;
  }
  a->textBegin = (uint64_t)(lo + k);
  a->numOps = numOps;
  if (ops && numOps <= c->maxOps)
    for (uint32_t q = 0; q < numOps / 2u; q++) {
      const uint32_t other = ops[numOps - 1u - q];
      ops[numOps - 1u - q] = ops[q];
      ops[q] = other;
    }
  return 1;
}

/* the status of read r, or its alignment (then < AWFM_ALIGN_OVERHANG) */
static uint32_t awfmAlignOne(struct awfmAlignCtx *c, uint64_t r, uint8_t **table, size_t *tableBytes, struct awfmAlignment *a) {
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
  if (hi < 0 || lo + (__int128)n > (__int128)b.L) return AWFM_ALIGN_OVERHANG;
  uint32_t *ops = c->out->ops ? c->out->ops + r * c->maxOps : NULL;
  if (!awfmAlignRead(c, in->readChars + readBegin, (int64_t)n, c->text + b.S, b.L, (int64_t)lo, (int64_t)hi, table, tableBytes, ops, a)) {
    c->failed = 1;
    return AWFM_VERIFY_NONE;
  }
  return a->distance;
}

static void awfmAlignRange(void *p, uint64_t begin, uint64_t end, unsigned tid) {
  struct awfmAlignCtx *c = p;
  uint8_t *table = NULL;
  size_t tableBytes = 0;
  uint64_t unaligned = 0, truncated = 0;
  for (uint64_t r = begin; r < end; r++) {
    struct awfmAlignment a = {0, 0, 0, 0};
    const uint32_t value = awfmAlignOne(c, r, &table, &tableBytes, &a);
    if (value >= AWFM_ALIGN_OVERHANG) {
      memset(&a, 0, sizeof a);
      if (value != AWFM_VERIFY_NONE) unaligned++;
    } else if (a.numOps > c->maxOps) {
      truncated++;
    }
    if (c->out->editDistances) c->out->editDistances[r] = value;
    if (c->out->textBegins) c->out->textBegins[r] = a.textBegin;
    if (c->out->textEnds) c->out->textEnds[r] = a.textEnd;
    if (c->out->numOps) c->out->numOps[r] = a.numOps;
  }
  free(table);
  c->unaligned[tid & 63u] += unaligned;
  c->truncated[tid & 63u] += truncated;
}

enum AwFmReturnCode awfmAlignChains(const struct AwFmVerifyInputs *in, const uint32_t *slots, uint64_t numReads, uint32_t maxCandidates,
                                    uint32_t bandPad, uint32_t maxDrift, uint32_t maxOps, const uint8_t *text, uint64_t length,
                                    const uint64_t *sequenceEnds, uint64_t numRecords, enum AwFmAlphabetType alphabet,
                                    const struct AwFmAlignOutputs *out, unsigned threads) {
  if (numReads == 0) return AwFmSuccess;
  const enum AwFmReturnCode rc = awfmBandCheckArguments(in, out && slots, text, length, sequenceEnds, numRecords, numReads, maxCandidates, bandPad, maxDrift);
  if (rc != AwFmSuccess) return rc;
  if (maxOps < 1 || maxOps > AWFM_ALIGN_MAX_OPS) return AwFmIllegalPositionError;
  struct awfmAlignCtx ctx;
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
  ctx.amino = alphabet == AwFmAlphabetAmino;
  awfmParallelFor(threads ? threads : 1, numReads, awfmAlignRange, &ctx);
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
