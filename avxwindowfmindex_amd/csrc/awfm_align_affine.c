/*
 * awfm_align_affine.c -- awfmAlignChainsAffine (include/awfm_gpu.h, "affine alignment"): the banded local alignment with affine
 * gap costs of every read against the record its chosen slot names, with soft clipping and the edit script.  The host twin of
 * awfmGpuAlignChainsAffine and its checker: a read at a time, the recurrence as the header states it with three rows of at most
 * 64 cells and a trace byte per cell in an n x width table, then the walk back through the three states.  Exact and readable
 * rather than fast.  The reference has no analogue (it stops at positions: ref src/AwFmParallelSearch.c:315-365).
 */
#include <stdlib.h>
#include <string.h>

#include "awfm_gpu.h"
#include "awfm_internal.h"

#define AWFM_AFFINE_NEG INT32_MIN /* minus infinity: awfmAffineMinus keeps it what it is */
/* a trace byte: the source of H in its low three bits, then whether F and E of the cell open their gap at its neighbour */
enum { AWFM_SRC_STOP = 0, AWFM_SRC_EQ = 1, AWFM_SRC_X = 2, AWFM_SRC_F = 3, AWFM_SRC_E = 4, AWFM_TRACE_F_OPENS = 8, AWFM_TRACE_E_OPENS = 16 };
enum { AWFM_OP_I = 1, AWFM_OP_D = 2, AWFM_OP_S = 4, AWFM_OP_EQ = 7, AWFM_OP_X = 8 };
enum { AWFM_STATE_H, AWFM_STATE_F, AWFM_STATE_E };

struct awfmAffineCtx {
  const struct AwFmVerifyInputs *in;
  const struct AwFmAffineOutputs *out;
  const uint32_t *chosen;
  const uint8_t *text;
  const uint64_t *ends;
  uint64_t length, numRecords;
  uint32_t slots, pad, drift, proper, maxOps;
  int32_t match, mismatch, open, extend;
  int amino, failed;
  uint64_t unaligned[64], truncated[64]; /* per thread of the loop */
};

struct awfmAffineAlignment {
  uint32_t score, distance, readBegin, readEnd, numOps;
  uint64_t textBegin, textEnd;
};

static uint32_t awfmAffineSub(const struct awfmAffineCtx *c, uint8_t a, uint8_t b) {
  const uint8_t x = c->amino ? awfmAminoAsciiToIndex(a) : awfmNucAsciiToIndex(a);
  const uint8_t y = c->amino ? awfmAminoAsciiToIndex(b) : awfmNucAsciiToIndex(b);
  return x == y && x < c->proper ? 0u : 1u;
}

static int32_t awfmAffineMinus(int32_t value, int32_t cost) { return value == AWFM_AFFINE_NEG ? AWFM_AFFINE_NEG : value - cost; }
static int32_t awfmAffineMax(int32_t a, int32_t b) { return a > b ? a : b; }

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
  int32_t rowsH[2][AWFM_VERIFY_MAX_BAND], rowsF[2][AWFM_VERIFY_MAX_BAND], E[AWFM_VERIFY_MAX_BAND];
  const int64_t width = hi - lo + 1;
  memset(a, 0, sizeof *a);
  if (n == 0 || n + hi < 0 || lo + 1 > L) return 1; /* no existing cell with i >= 1 */
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
  int32_t *prevH = rowsH[0], *curH = rowsH[1], *prevF = rowsF[0], *curF = rowsF[1];
  const int32_t open = c->open + c->extend, extend = c->extend;
  for (int64_t k = 0; k < width; k++) { /* row 0 */
    const int64_t t = lo + k;
    prevH[k] = t >= 0 && t <= L ? 0 : AWFM_AFFINE_NEG;
    prevF[k] = AWFM_AFFINE_NEG;
  }
  int32_t best = 0;
  int64_t bestI = 0, bestK = 0;
  for (int64_t i = 1; i <= n; i++) {
    for (int64_t k = 0; k < width; k++) {
      const int64_t t = i + lo + k;
      uint8_t code = AWFM_SRC_STOP;
      curH[k] = curF[k] = E[k] = AWFM_AFFINE_NEG;
      if (t >= 0 && t <= L) {
        /* (i-1, t-1) lies on the same diagonal, (i-1, t) on the next one up, (i, t-1) on the one below */
        const uint32_t sub = t >= 1 ? awfmAffineSub(c, R[i - 1], T[t - 1]) : 1u;
        const int32_t M = t >= 1 ? awfmAffineMinus(prevH[k], sub ? c->mismatch : -c->match) : AWFM_AFFINE_NEG;
        const int32_t fOpens = awfmAffineMinus(k + 1 < width ? prevH[k + 1] : AWFM_AFFINE_NEG, open);
        const int32_t fExtends = awfmAffineMinus(k + 1 < width ? prevF[k + 1] : AWFM_AFFINE_NEG, extend);
        const int32_t eOpens = awfmAffineMinus(k >= 1 ? curH[k - 1] : AWFM_AFFINE_NEG, open);
        const int32_t eExtends = awfmAffineMinus(k >= 1 ? E[k - 1] : AWFM_AFFINE_NEG, extend);
        const int32_t F = awfmAffineMax(fOpens, fExtends), e = awfmAffineMax(eOpens, eExtends);
        const int32_t H = awfmAffineMax(awfmAffineMax(0, M), awfmAffineMax(F, e));
        curH[k] = H;
        curF[k] = F;
        E[k] = e;
        code = H == 0 ? AWFM_SRC_STOP : M == H ? (sub ? AWFM_SRC_X : AWFM_SRC_EQ) : F == H ? AWFM_SRC_F : AWFM_SRC_E;
        code |= (fOpens >= fExtends ? AWFM_TRACE_F_OPENS : 0) | (eOpens >= eExtends ? AWFM_TRACE_E_OPENS : 0);
        if (H > best) { /* rows in ascending order, then columns: the smallest i, then the smallest t of the largest H */
          best = H;
          bestI = i;
          bestK = k;
        }
      }
      trace[(i - 1) * width + k] = code;
    }
    int32_t *swap = prevH;
    prevH = curH;
    curH = swap;
    swap = prevF;
    prevF = curF;
    curF = swap;
  }
  if (best == 0) return 1;
  a->score = (uint32_t)best;
  a->readEnd = (uint32_t)bestI;
  a->textEnd = (uint64_t)(bestI + lo + bestK);
  /* the walk meets the runs last to first: they are written in that order and turned round */
  struct awfmAffineRuns runs = {ops, c->maxOps, 0, 0, 0};
  awfmAffineEmit(&runs, AWFM_OP_S, (uint32_t)(n - bestI));
  int64_t i = bestI, k = bestK;
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
  const uint64_t at = r * c->slots + j;
  const uint32_t s = in->sequences[at];
  if (s == AWFM_CANDIDATES_NONE || in->chainAnchors[at] == 0) return AWFM_VERIFY_NONE;
  const uint64_t readBegin = in->readOffsets[r], readEnd = in->readOffsets[r + 1];
  if (readBegin > readEnd || readEnd > in->numReadChars) return AWFM_VERIFY_MALFORMED;
  const uint64_t rb = in->chainReadBegins[at], re = in->chainReadEnds[at], n = readEnd - readBegin;
  if (rb > re || re > n) return AWFM_VERIFY_MALFORMED;
  if (s >= (c->numRecords ? c->numRecords : 1u)) return AWFM_VERIFY_MALFORMED;
  const uint64_t S = c->numRecords && s ? c->ends[s - 1] + 1u : 0u, E = c->numRecords ? c->ends[s] : c->length;
  if (c->numRecords && s && S == 0) return AWFM_VERIFY_MALFORMED; /* (an end of 2^64 - 1) */
  if (E < S || E > c->length) return AWFM_VERIFY_MALFORMED;
  const int64_t bD = in->chainBeginDiagonals[at], eD = in->chainEndDiagonals[at];
  const __int128 tb = (__int128)rb + bD, te = (__int128)re + eD;
  if (tb < 0 || tb > te || te > (__int128)(E - S)) return AWFM_VERIFY_MALFORMED;
  /* 0 <= tb <= te <= L < 2^63 and rb, re < 2^32: both diagonals lie in (-2^32, 2^63) and their difference is exact */
  const __int128 delta = (__int128)eD - bD;
  if (delta > (__int128)c->drift || delta < -(__int128)c->drift) return AWFM_VERIFY_TOO_WIDE;
  if (n > AWFM_ALIGN_MAX_LENGTH) return AWFM_VERIFY_TOO_LONG;
  const int64_t L = (int64_t)(E - S);
  const __int128 lo = (bD < eD ? bD : eD) - (__int128)c->pad, hi = (bD > eD ? bD : eD) + (__int128)c->pad;
  uint32_t *ops = c->out->ops ? c->out->ops + r * c->maxOps : NULL;
  if (!awfmAffineRead(c, in->readChars + readBegin, (int64_t)n, c->text + S, L, (int64_t)lo, (int64_t)hi, table, tableBytes, ops, a)) {
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

enum AwFmReturnCode awfmAlignChainsAffine(const struct AwFmVerifyInputs *in, const uint32_t *slots, uint64_t numReads,
                                          uint32_t maxCandidates, uint32_t bandPad, uint32_t maxDrift,
                                          const struct AwFmAlignScoring *scoring, uint32_t maxOps, const uint8_t *text, uint64_t length,
                                          const uint64_t *sequenceEnds, uint64_t numRecords, enum AwFmAlphabetType alphabet,
                                          const struct AwFmAffineOutputs *out, unsigned threads) {
  if (numReads == 0) return AwFmSuccess;
  if (!in || !out || !slots || !scoring || !in->readOffsets || !in->sequences || !in->chainAnchors || !in->chainReadBegins ||
      !in->chainReadEnds || !in->chainBeginDiagonals || !in->chainEndDiagonals)
    return AwFmNullPtrError;
  if ((!in->readChars && in->numReadChars != 0) || (!text && length != 0) || (!sequenceEnds && numRecords != 0)) return AwFmNullPtrError;
  if (numReads >= (1ull << 32) || maxCandidates < 1 || maxCandidates > AWFM_CANDIDATES_MAX_SLOTS) return AwFmIllegalPositionError;
  if ((uint64_t)maxDrift + 2ull * bandPad + 1ull > AWFM_VERIFY_MAX_BAND) return AwFmIllegalPositionError;
  if (maxOps < 1 || maxOps > AWFM_ALIGN_MAX_OPS) return AwFmIllegalPositionError;
  if (scoring->match < 1 || scoring->match > 255 || scoring->mismatch > 255 || scoring->gapOpen > 255 || scoring->gapExtend < 1 ||
      scoring->gapExtend > 255)
    return AwFmIllegalPositionError;
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
  ctx.match = (int32_t)scoring->match;
  ctx.mismatch = (int32_t)scoring->mismatch;
  ctx.open = (int32_t)scoring->gapOpen;
  ctx.extend = (int32_t)scoring->gapExtend;
  ctx.amino = alphabet == AwFmAlphabetAmino;
  ctx.proper = ctx.amino ? 20u : 4u;
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
