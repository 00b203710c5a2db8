/*
 * awfm_strands.c -- awfmChooseStrands and awfmOrientReads (include/awfm_gpu.h, "strands"): per read or pair the strand and slot
 * among the 2C strand slots of a read searched as sequenced and reverse-complemented, the qualities, the pairing of mates from
 * opposite strands and the rescue windows by row; and the gather of the chosen strands into one batch.  The host twins of
 * awfmGpuChooseStrands and awfmGpuOrientReads and their checkers: a read or pair at a time, every candidate (u1, u2) in turn,
 * the header's rules as written.  Exact and readable rather than fast.  The reference has no analogue (it stops at positions:
 * ref src/AwFmParallelSearch.c:315-365).
 */
#include <stdlib.h>
#include <string.h>

#include "awfm_gpu.h"
#include "awfm_internal.h"

#define AWFM_STRAND_SLOTS (2 * AWFM_CANDIDATES_MAX_SLOTS)
#define AWFM_STRAND_NONE 0xFFFFFFFFu /* no strand slot */

struct awfmStrandCtx {
  const struct AwFmStrandInputs *in;
  const struct AwFmStrandOutputs *out;
  const struct AwFmPairParams *params;
  uint64_t numReads;
  uint32_t slots, paired;
  uint64_t reverse[64], proper[64], windows[64], malformed[64]; /* per thread of the loop */
};

struct awfmStrandSlot {
  int counts;
  uint32_t score, sequence, readEnd;
  uint64_t textEnd;
  int64_t start;
};

/* what rules 1 to 5 make of one read */
struct awfmStrandRead {
  struct awfmStrandSlot slot[AWFM_STRAND_SLOTS];
  int malformed;
  int64_t n;
  uint32_t best, bestScore, secondScore, quality;
};

struct awfmStrandCandidate {
  int exists, concordant;
  uint32_t u1, u2;
  uint64_t value;
  int64_t length;
};

static int64_t awfmStrandAdd(int64_t x, int64_t y) { return (int64_t)((uint64_t)x + (uint64_t)y); }
static int64_t awfmStrandSub(int64_t x, int64_t y) { return (int64_t)((uint64_t)x - (uint64_t)y); }
static uint64_t awfmStrandRaised(int64_t x) { return x < 0 ? 0u : (uint64_t)x; }

/* rule 3, and a strand slot is the same as itself */
static int awfmStrandSame(const struct awfmStrandSlot *slot, uint32_t C, uint32_t u, uint32_t v) {
  if (u == v) return 1;
  return u / C == v / C && slot[u].counts && slot[v].counts && slot[u].sequence == slot[v].sequence && slot[u].readEnd == slot[v].readEnd &&
         slot[u].textEnd == slot[v].textEnd;
}

/* rules 1 to 5 */
static void awfmStrandLoad(const struct awfmStrandCtx *c, uint64_t r, struct awfmStrandRead *read) {
  const struct AwFmStrandInputs *in = c->in;
  const uint32_t C = c->slots, floor = c->params->minScore > 1u ? c->params->minScore : 1u;
  const uint64_t rows[2] = {r, c->numReads + r};
  const uint64_t forwardBegin = in->readOffsets[rows[0]], forwardEnd = in->readOffsets[rows[0] + 1u];
  const uint64_t reverseBegin = in->readOffsets[rows[1]], reverseEnd = in->readOffsets[rows[1] + 1u];
  read->malformed = forwardBegin > forwardEnd || reverseBegin > reverseEnd || forwardEnd - forwardBegin != reverseEnd - reverseBegin;
  read->n = (int64_t)(forwardEnd - forwardBegin);
  read->best = AWFM_STRAND_NONE;
  for (uint32_t u = 0; u < 2u * C; u++) {
    struct awfmStrandSlot *s = &read->slot[u];
    const uint64_t at = rows[u / C] * C + u % C;
    s->score = in->slotScores[at];
    s->sequence = in->sequences[at];
    s->readEnd = in->slotReadEnds[at];
    s->textEnd = in->slotTextEnds[at];
    s->start = awfmStrandSub((int64_t)s->textEnd, (int64_t)s->readEnd);
    s->counts = !read->malformed && s->score < AWFM_VERIFY_TOO_LONG && s->score >= floor;
    if (s->counts && (read->best == AWFM_STRAND_NONE || s->score > read->slot[read->best].score)) read->best = u;
  }
  read->bestScore = read->secondScore = read->quality = 0;
  if (read->best == AWFM_STRAND_NONE) return;
  read->bestScore = read->slot[read->best].score;
  for (uint32_t u = 0; u < 2u * C; u++)
    if (read->slot[u].counts && !awfmStrandSame(read->slot, C, u, read->best) && read->slot[u].score > read->secondScore)
      read->secondScore = read->slot[u].score;
  read->quality = (uint32_t)((uint64_t)c->params->mapqCap * (read->bestScore - read->secondScore) / read->bestScore);
}

/* candidate x goes before candidate y: the larger value, then the concordant one, then the lowest u1, then the lowest u2 */
static int awfmStrandBefore(const struct awfmStrandCandidate *x, const struct awfmStrandCandidate *y) {
  if (!y->exists) return 1;
  if (x->value != y->value) return x->value > y->value;
  if (x->concordant != y->concordant) return x->concordant;
  if (x->u1 != y->u1) return x->u1 < y->u1;
  return x->u2 < y->u2;
}

/* the per-read and per-row outputs of read r: its chosen strand slot, its quality and the window it was given */
static void awfmStrandStore(struct awfmStrandCtx *c, uint64_t r, const struct awfmStrandRead *read, uint32_t chosen, uint32_t quality,
                            int windowStrand, uint32_t windowSequence, uint64_t windowBegin, uint64_t windowEnd, uint64_t *reverse) {
  const struct AwFmStrandOutputs *out = c->out;
  const uint32_t C = c->slots;
  const uint32_t strand = chosen == AWFM_STRAND_NONE ? 0u : chosen / C, slot = chosen == AWFM_STRAND_NONE ? AWFM_CHAINS_NO_SLOT : chosen % C;
  *reverse += strand;
  if (out->strands) out->strands[r] = (uint8_t)strand;
  if (out->strandSlots) out->strandSlots[r] = slot;
  if (out->bestScores) out->bestScores[r] = read->bestScore;
  if (out->secondScores) out->secondScores[r] = read->secondScore;
  if (out->mappingQualities) out->mappingQualities[r] = (uint8_t)quality;
  if (out->baseFlags) out->baseFlags[r] = strand ? 0x10u : 0u;
  for (uint32_t sigma = 0; sigma < 2u; sigma++) {
    const uint64_t row = sigma * c->numReads + r;
    const int here = windowStrand == (int)sigma;
    if (out->rowSlots) out->rowSlots[row] = chosen != AWFM_STRAND_NONE && strand == sigma ? slot : AWFM_CHAINS_NO_SLOT;
    if (out->windowSequences) out->windowSequences[row] = here ? windowSequence : AWFM_CANDIDATES_NONE;
    if (out->windowBegins) out->windowBegins[row] = here ? windowBegin : 0u;
    if (out->windowEnds) out->windowEnds[row] = here ? windowEnd : 0u;
  }
}

static void awfmStrandReadRange(void *ctx, uint64_t begin, uint64_t end, unsigned tid) {
  struct awfmStrandCtx *c = ctx;
  uint64_t reverse = 0, malformed = 0;
  for (uint64_t r = begin; r < end; r++) {
    struct awfmStrandRead read;
    awfmStrandLoad(c, r, &read);
    malformed += (uint64_t)read.malformed;
    awfmStrandStore(c, r, &read, read.best, read.quality, -1, AWFM_CANDIDATES_NONE, 0, 0, &reverse);
  }
  c->reverse[tid & 63u] += reverse;
  c->malformed[tid & 63u] += malformed;
}

static void awfmStrandPairRange(void *ctx, uint64_t begin, uint64_t end, unsigned tid) {
  struct awfmStrandCtx *c = ctx;
  const struct AwFmStrandOutputs *out = c->out;
  const struct AwFmPairParams *q = c->params;
  const uint32_t C = c->slots;
  uint64_t reverse = 0, proper = 0, windows = 0, malformed = 0;
  for (uint64_t p = begin; p < end; p++) {
    struct awfmStrandRead read[2];
    for (int m = 0; m < 2; m++) {
      awfmStrandLoad(c, 2u * p + (uint64_t)m, &read[m]);
      malformed += (uint64_t)read[m].malformed;
    }
    /* 6, 7: every candidate, and 8: the one that goes before all others */
    struct awfmStrandCandidate all[2 * AWFM_CANDIDATES_MAX_SLOTS * AWFM_CANDIDATES_MAX_SLOTS + 1], winner;
    unsigned numAll = 0;
    memset(&winner, 0, sizeof winner);
    for (uint32_t u1 = 0; u1 < 2u * C; u1++)
      for (uint32_t u2 = 0; u2 < 2u * C; u2++) {
        const struct awfmStrandSlot *x = &read[0].slot[u1], *y = &read[1].slot[u2];
        if (!x->counts || !y->counts) continue;
        struct awfmStrandCandidate k = {1, 0, u1, u2, (uint64_t)x->score + y->score, 0};
        if (u1 / C != u2 / C) {
          const int firstIsA = u1 / C == 0; /* A is the one on strand 0, B the one on strand 1 */
          const struct awfmStrandSlot *A = firstIsA ? x : y, *B = firstIsA ? y : x;
          k.length = awfmStrandSub(awfmStrandAdd(B->start, firstIsA ? read[1].n : read[0].n), A->start);
          k.concordant = x->sequence == y->sequence && q->minInsert <= k.length && k.length <= q->maxInsert;
        }
        if (!k.concordant) {
          if (u1 != read[0].best || u2 != read[1].best) continue;
          k.value = k.value > q->unpairedPenalty ? k.value - q->unpairedPenalty : 0u;
        }
        all[numAll++] = k;
      }
    for (unsigned i = 0; i < numAll; i++)
      if (awfmStrandBefore(&all[i], &winner)) winner = all[i];
    /* pair mates' rule 5: the largest value among the others that are not the winner's alignments again */
    uint64_t second = 0;
    for (unsigned i = 0; i < numAll; i++) {
      const struct awfmStrandCandidate *k = &all[i];
      if (awfmStrandSame(read[0].slot, C, k->u1, winner.u1) && awfmStrandSame(read[1].slot, C, k->u2, winner.u2)) continue;
      if (k->value > second) second = k->value;
    }
    const int isProper = winner.exists && winner.concordant;
    uint32_t chosen[2] = {read[0].best, read[1].best}; /* (one mate placed or none: what each has) */
    uint64_t value = 0;
    if (winner.exists) {
      chosen[0] = winner.u1;
      chosen[1] = winner.u2;
      value = winner.value;
    } else if (read[0].best != AWFM_STRAND_NONE) {
      value = read[0].bestScore;
    } else if (read[1].best != AWFM_STRAND_NONE) {
      value = read[1].bestScore;
    }
    const uint64_t quality = isProper ? (uint64_t)q->mapqCap * (winner.value - second) / winner.value : 0u;
    proper += (uint64_t)isProper;
    if (out->properPairs) out->properPairs[p] = (uint8_t)isProper;
    if (out->pairScores) out->pairScores[p] = (uint32_t)value;
    if (out->pairSecondScores) out->pairSecondScores[p] = (uint32_t)second;
    if (out->templateLengths) out->templateLengths[p] = isProper ? winner.length : 0;
    if (out->pairQualities) out->pairQualities[p] = (uint8_t)quality;
    for (int m = 0; m < 2; m++) {
      const struct awfmStrandRead *mine = &read[m], *mate = &read[1 - m];
      uint64_t mapq = mine->quality; /* (0 without a best) */
      if (isProper) {
        mapq = chosen[m] == mine->best ? mine->quality : 0u;
        if (quality > mapq) mapq = quality;
      }
      /* 10: a read of a pair that is not proper, in the window its mate's best strand slot names, on the other strand */
      int windowStrand = -1;
      uint32_t windowSequence = AWFM_CANDIDATES_NONE;
      uint64_t windowBegin = 0, windowEnd = 0;
      if (!isProper && mate->best != AWFM_STRAND_NONE) {
        const struct awfmStrandSlot *s = &mate->slot[mate->best];
        const int64_t pad = (int64_t)q->windowPad;
        windowSequence = s->sequence;
        if (mate->best / C == 0) {
          windowStrand = 1;
          windowBegin = awfmStrandRaised(awfmStrandSub(awfmStrandSub(awfmStrandAdd(s->start, q->minInsert), mine->n), pad));
          windowEnd = awfmStrandRaised(awfmStrandAdd(awfmStrandAdd(s->start, q->maxInsert), pad));
        } else {
          const int64_t E = awfmStrandAdd(s->start, mate->n);
          windowStrand = 0;
          windowBegin = awfmStrandRaised(awfmStrandSub(awfmStrandSub(E, q->maxInsert), pad));
          windowEnd = awfmStrandRaised(awfmStrandAdd(awfmStrandAdd(awfmStrandSub(E, q->minInsert), mine->n), pad));
        }
        windows++;
      }
      awfmStrandStore(c, 2u * p + (uint64_t)m, mine, chosen[m], (uint32_t)mapq, windowStrand, windowSequence, windowBegin, windowEnd, &reverse);
    }
  }
  c->reverse[tid & 63u] += reverse;
  c->proper[tid & 63u] += proper;
  c->windows[tid & 63u] += windows;
  c->malformed[tid & 63u] += malformed;
}

enum AwFmReturnCode awfmChooseStrands(const struct AwFmStrandInputs *in, uint64_t numReads, uint32_t maxCandidates, uint32_t flags,
                                      const struct AwFmPairParams *params, const struct AwFmStrandOutputs *out, unsigned threads) {
  if (numReads == 0) return AwFmSuccess;
  if (!in || !out || !params || !in->readOffsets || !in->sequences || !in->slotScores || !in->slotReadEnds || !in->slotTextEnds)
    return AwFmNullPtrError;
  if (maxCandidates < 1 || maxCandidates > AWFM_CANDIDATES_MAX_SLOTS || numReads >= (1ull << 31)) return AwFmIllegalPositionError;
  if ((flags & ~AWFM_STRANDS_PAIRED) != 0 || ((flags & AWFM_STRANDS_PAIRED) && (numReads & 1u))) return AwFmIllegalPositionError;
  if ((flags & AWFM_STRANDS_PAIRED) &&
      (params->minInsert > params->maxInsert || params->minInsert < -AWFM_PAIR_MAX_INSERT || params->maxInsert > AWFM_PAIR_MAX_INSERT))
    return AwFmIllegalPositionError;
  if (params->mapqCap > AWFM_SCORE_MAX_MAPQ) return AwFmIllegalPositionError;
  struct awfmStrandCtx context, *ctx = &context;
  memset(ctx, 0, sizeof *ctx);
  ctx->in = in;
  ctx->out = out;
  ctx->params = params;
  ctx->numReads = numReads;
  ctx->slots = maxCandidates;
  ctx->paired = flags & AWFM_STRANDS_PAIRED;
  if (ctx->paired) awfmParallelFor(threads ? threads : 1, numReads / 2u, awfmStrandPairRange, ctx);
  else awfmParallelFor(threads ? threads : 1, numReads, awfmStrandReadRange, ctx);
  uint64_t reverse = 0, proper = 0, windows = 0, malformed = 0;
  for (unsigned t = 0; t < 64; t++) {
    reverse += ctx->reverse[t];
    proper += ctx->proper[t];
    windows += ctx->windows[t];
    malformed += ctx->malformed[t];
  }
  if (out->numReverse) *out->numReverse += reverse;
  if (out->numProper) *out->numProper += proper;
  if (out->numWindows) *out->numWindows += windows;
  if (out->numMalformed) *out->numMalformed += malformed;
  return AwFmSuccess;
}

struct awfmOrientCtx {
  const struct AwFmOrientInputs *in;
  const struct AwFmOrientOutputs *out;
  uint64_t numReads;
  uint32_t slots;
  uint64_t malformed[64];
};

static void awfmOrientRange(void *ctx, uint64_t begin, uint64_t end, unsigned tid) {
  struct awfmOrientCtx *c = ctx;
  const struct AwFmOrientInputs *in = c->in;
  const struct AwFmOrientOutputs *out = c->out;
  const uint64_t *offsets = in->rows.readOffsets, numChars = in->rows.numReadChars, R = c->numReads;
  const uint32_t C = c->slots;
  uint64_t malformed = 0;
  for (uint64_t r = begin; r < end; r++) {
    const uint64_t forwardBegin = offsets[r], forwardEnd = offsets[r + 1u], reverseBegin = offsets[R + r], reverseEnd = offsets[R + r + 1u];
    const uint64_t n = forwardEnd - forwardBegin, to = forwardBegin - offsets[0];
    const uint32_t strand = in->strands[r];
    const int good = forwardBegin <= forwardEnd && forwardEnd <= numChars && reverseBegin <= reverseEnd && reverseEnd <= numChars &&
                     reverseEnd - reverseBegin == n && strand <= 1u && forwardBegin >= offsets[0] && forwardEnd - offsets[0] <= out->capacity;
    out->readOffsets[r] = to;
    if (r + 1u == R) out->readOffsets[R] = forwardEnd - offsets[0];
    malformed += (uint64_t)!good;
    if (good) {
      const uint64_t from = strand ? reverseBegin : forwardBegin;
      for (uint64_t i = 0; i < n; i++) out->readChars[to + i] = in->rows.readChars[from + i];
      if (out->qualities)
        for (uint64_t i = 0; i < n; i++) out->qualities[to + i] = in->qualities[forwardBegin + (strand ? n - 1u - i : i)];
    }
    const uint64_t row = good ? strand * R + r : 0u;
    for (uint32_t j = 0; j < C; j++) {
      const uint64_t at = r * C + j, source = row * C + j;
      if (out->sequences) out->sequences[at] = good ? in->rows.sequences[source] : AWFM_CANDIDATES_NONE;
      if (out->chainAnchors) out->chainAnchors[at] = good ? in->rows.chainAnchors[source] : 0u;
      if (out->chainReadBegins) out->chainReadBegins[at] = good ? in->rows.chainReadBegins[source] : 0u;
      if (out->chainReadEnds) out->chainReadEnds[at] = good ? in->rows.chainReadEnds[source] : 0u;
      if (out->chainBeginDiagonals) out->chainBeginDiagonals[at] = good ? in->rows.chainBeginDiagonals[source] : 0;
      if (out->chainEndDiagonals) out->chainEndDiagonals[at] = good ? in->rows.chainEndDiagonals[source] : 0;
      if (out->slotScores) out->slotScores[at] = good ? in->slotScores[source] : AWFM_VERIFY_NONE;
      if (out->slotReadEnds) out->slotReadEnds[at] = good ? in->slotReadEnds[source] : 0u;
      if (out->slotTextEnds) out->slotTextEnds[at] = good ? in->slotTextEnds[source] : 0u;
    }
  }
  c->malformed[tid & 63u] += malformed;
}

static int awfmOrientOverlap(const void *x, uint64_t xBytes, const void *y, uint64_t yBytes) {
  return x && y && xBytes && yBytes && (uintptr_t)x < (uintptr_t)y + yBytes && (uintptr_t)y < (uintptr_t)x + xBytes;
}

enum AwFmReturnCode awfmOrientReads(const struct AwFmOrientInputs *in, uint64_t numReads, uint32_t maxCandidates,
                                    const struct AwFmOrientOutputs *out, unsigned threads) {
  if (numReads == 0) return AwFmSuccess;
  if (!in || !out || !in->rows.readOffsets || !in->strands || !out->readOffsets || (!in->rows.readChars && in->rows.numReadChars != 0) ||
      (!out->readChars && out->capacity != 0))
    return AwFmNullPtrError;
  if (!in->qualities != !out->qualities || !in->rows.sequences != !out->sequences || !in->rows.chainAnchors != !out->chainAnchors ||
      !in->rows.chainReadBegins != !out->chainReadBegins || !in->rows.chainReadEnds != !out->chainReadEnds ||
      !in->rows.chainBeginDiagonals != !out->chainBeginDiagonals || !in->rows.chainEndDiagonals != !out->chainEndDiagonals ||
      !in->slotScores != !out->slotScores || !in->slotReadEnds != !out->slotReadEnds || !in->slotTextEnds != !out->slotTextEnds)
    return AwFmNullPtrError;
  if (maxCandidates < 1 || maxCandidates > AWFM_CANDIDATES_MAX_SLOTS || numReads >= (1ull << 31)) return AwFmIllegalPositionError;
  if (awfmOrientOverlap(in->rows.readChars, in->rows.numReadChars, out->readChars, out->capacity) ||
      awfmOrientOverlap(in->qualities, in->rows.numReadChars, out->qualities, out->capacity))
    return AwFmIllegalPositionError;
  struct awfmOrientCtx ctx;
  memset(&ctx, 0, sizeof ctx);
  ctx.in = in;
  ctx.out = out;
  ctx.numReads = numReads;
  ctx.slots = maxCandidates;
  awfmParallelFor(threads ? threads : 1, numReads, awfmOrientRange, &ctx);
  uint64_t malformed = 0;
  for (unsigned t = 0; t < 64; t++) malformed += ctx.malformed[t];
  if (out->numMalformed) *out->numMalformed += malformed;
  return AwFmSuccess;
}
