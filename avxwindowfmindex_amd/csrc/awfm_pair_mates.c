/*
 * awfm_pair_mates.c -- awfmPairMates and awfmReverseComplementReads (include/awfm_gpu.h, "pair mates"): per pair of reads the
 * winner among the concordant slot pairs and the discordant candidate, the second, the pair's quality, the reads' qualities and
 * the rescue windows; and the reverse complement of reads where they lie.  The host twins of awfmGpuPairMates and
 * awfmGpuReverseComplementReads and their checkers: a pair at a time, every candidate (a, b) in turn, the header's rules as
 * written.  Exact and readable rather than fast.  The reference has no analogue (it stops at positions:
 * ref src/AwFmParallelSearch.c:315-365).
 */
#include <stdlib.h>
#include <string.h>

#include "awfm_gpu.h"
#include "awfm_internal.h"

struct awfmPairCtx {
  const struct AwFmPairInputs *in;
  const struct AwFmPairOutputs *out;
  const struct AwFmPairParams *params;
  uint32_t slots;
  uint64_t proper[64], windows[64]; /* per thread of the loop */
};

struct awfmPairSlot {
  int counts;
  uint32_t score, sequence, readEnd;
  uint64_t textEnd;
  int64_t start;
};

struct awfmPairCandidate {
  int exists, concordant;
  uint32_t a, b;
  uint64_t value;
};

/* sums of positions are 64-bit two's complement */
static int64_t awfmPairAdd(int64_t x, int64_t y) { return (int64_t)((uint64_t)x + (uint64_t)y); }
static int64_t awfmPairSub(int64_t x, int64_t y) { return (int64_t)((uint64_t)x - (uint64_t)y); }
static uint64_t awfmPairRaised(int64_t x) { return x < 0 ? 0u : (uint64_t)x; }

/* candidate x goes before candidate y: the larger value, then the concordant one, then the lowest a, then the lowest b */
static int awfmPairBefore(const struct awfmPairCandidate *x, const struct awfmPairCandidate *y) {
  if (!y->exists) return 1;
  if (x->value != y->value) return x->value > y->value;
  if (x->concordant != y->concordant) return x->concordant;
  if (x->a != y->a) return x->a < y->a;
  return x->b < y->b;
}

static int awfmPairSame(const struct awfmPairSlot *slot, uint32_t j, uint32_t k) {
  if (j == k) return 1;
  return slot[j].counts && slot[k].counts && slot[j].sequence == slot[k].sequence && slot[j].readEnd == slot[k].readEnd &&
         slot[j].textEnd == slot[k].textEnd;
}

static void awfmPairRange(void *ctx, uint64_t begin, uint64_t end, unsigned tid) {
  struct awfmPairCtx *c = ctx;
  const struct AwFmPairInputs *in = c->in;
  const struct AwFmPairOutputs *out = c->out;
  const struct AwFmPairParams *q = c->params;
  const uint32_t C = c->slots, floor = q->minScore > 1u ? q->minScore : 1u;
  uint64_t proper = 0, windows = 0;
  for (uint64_t p = begin; p < end; p++) {
    const uint64_t reads[2] = {2u * p, 2u * p + 1u};
    struct awfmPairSlot slot[2][AWFM_CANDIDATES_MAX_SLOTS];
    int64_t n[2];
    uint32_t best[2];
    /* 1: the counting slots, their starts and each mate's best slot */
    for (int m = 0; m < 2; m++) {
      const uint64_t r = reads[m], readBegin = in->readOffsets[r], readEnd = in->readOffsets[r + 1u];
      n[m] = (int64_t)(readEnd - readBegin);
      best[m] = AWFM_CHAINS_NO_SLOT;
      for (uint32_t j = 0; j < C; j++) {
        struct awfmPairSlot *s = &slot[m][j];
        s->score = in->slotScores[r * C + j];
        s->sequence = in->sequences[r * C + j];
        s->readEnd = in->slotReadEnds[r * C + j];
        s->textEnd = in->slotTextEnds[r * C + j];
        s->start = awfmPairSub((int64_t)s->textEnd, (int64_t)s->readEnd);
        s->counts = readBegin <= readEnd && s->score < AWFM_VERIFY_TOO_LONG && s->score >= floor;
        if (s->counts && (best[m] == AWFM_CHAINS_NO_SLOT || s->score > slot[m][best[m]].score)) best[m] = j;
      }
    }
    /* 2, 3: every candidate, and 4: the one that goes before all others */
    struct awfmPairCandidate all[AWFM_CANDIDATES_MAX_SLOTS * AWFM_CANDIDATES_MAX_SLOTS + 1], winner;
    int64_t lengths[AWFM_CANDIDATES_MAX_SLOTS * AWFM_CANDIDATES_MAX_SLOTS + 1];
    unsigned numAll = 0;
    int64_t winnerLength = 0;
    memset(&winner, 0, sizeof winner);
    for (uint32_t a = 0; a < C; a++)
      for (uint32_t b = 0; b < C; b++) {
        const struct awfmPairSlot *x = &slot[0][a], *y = &slot[1][b];
        if (!x->counts || !y->counts) continue;
        const int64_t T = awfmPairSub(awfmPairAdd(y->start, n[1]), x->start);
        const int concordant = x->sequence == y->sequence && q->minInsert <= T && T <= q->maxInsert;
        struct awfmPairCandidate k = {1, concordant, a, b, (uint64_t)x->score + y->score};
        if (!concordant) {
          if (a != best[0] || b != best[1]) continue;
          k.value = k.value > q->unpairedPenalty ? k.value - q->unpairedPenalty : 0u;
        }
        lengths[numAll] = T;
        all[numAll++] = k;
      }
    for (unsigned i = 0; i < numAll; i++)
      if (awfmPairBefore(&all[i], &winner)) {
        winner = all[i];
        winnerLength = lengths[i];
      }
    /* 5: the largest value among the others that are not the winner's alignments again */
    uint64_t second = 0;
    for (unsigned i = 0; i < numAll; i++) {
      const struct awfmPairCandidate *k = &all[i];
      if (awfmPairSame(slot[0], k->a, winner.a) && awfmPairSame(slot[1], k->b, winner.b)) continue; /* (the winner itself too) */
      if (k->value > second) second = k->value;
    }
    const int isProper = winner.exists && winner.concordant;
    uint32_t chosen[2] = {best[0], best[1]}; /* (one mate placed or none: what each has) */
    uint64_t value = 0;
    if (winner.exists) {
      chosen[0] = winner.a;
      chosen[1] = winner.b;
      value = winner.value;
    } else if (best[0] != AWFM_CHAINS_NO_SLOT) {
      value = slot[0][best[0]].score;
    } else if (best[1] != AWFM_CHAINS_NO_SLOT) {
      value = slot[1][best[1]].score;
    }
    /* 6 */
    const uint64_t quality = isProper ? (uint64_t)q->mapqCap * (winner.value - second) / winner.value : 0u;
    proper += (uint64_t)isProper;
    if (out->properPairs) out->properPairs[p] = (uint8_t)isProper;
    if (out->pairScores) out->pairScores[p] = (uint32_t)value;
    if (out->pairSecondScores) out->pairSecondScores[p] = (uint32_t)second;
    if (out->templateLengths) out->templateLengths[p] = isProper ? winnerLength : 0;
    if (out->pairQualities) out->pairQualities[p] = (uint8_t)quality;
    for (int m = 0; m < 2; m++) {
      const uint64_t r = reads[m];
      const uint64_t given = in->mappingQualities ? in->mappingQualities[r] : 0u;
      uint64_t mine = best[m] == AWFM_CHAINS_NO_SLOT ? 0u : given;
      if (isProper) {
        mine = chosen[m] == best[m] ? given : 0u;
        if (quality > mine) mine = quality;
      }
      /* 7: a read of a pair that is not proper, in the window its mate's best slot names */
      const int other = 1 - m;
      uint32_t windowSequence = AWFM_CANDIDATES_NONE;
      uint64_t windowBegin = 0, windowEnd = 0;
      if (!isProper && best[other] != AWFM_CHAINS_NO_SLOT) {
        const struct awfmPairSlot *s = &slot[other][best[other]];
        const int64_t pad = (int64_t)q->windowPad;
        windowSequence = s->sequence;
        if (m == 1) {
          windowBegin = awfmPairRaised(awfmPairSub(awfmPairSub(awfmPairAdd(s->start, q->minInsert), n[1]), pad));
          windowEnd = awfmPairRaised(awfmPairAdd(awfmPairAdd(s->start, q->maxInsert), pad));
        } else {
          const int64_t E = awfmPairAdd(s->start, n[1]);
          windowBegin = awfmPairRaised(awfmPairSub(awfmPairSub(E, q->maxInsert), pad));
          windowEnd = awfmPairRaised(awfmPairAdd(awfmPairAdd(awfmPairSub(E, q->minInsert), n[0]), pad));
        }
        windows++;
      }
      if (out->pairSlots) out->pairSlots[r] = chosen[m];
      if (out->mappingQualities) out->mappingQualities[r] = (uint8_t)mine;
      if (out->windowSequences) out->windowSequences[r] = windowSequence;
      if (out->windowBegins) out->windowBegins[r] = windowBegin;
      if (out->windowEnds) out->windowEnds[r] = windowEnd;
    }
  }
  c->proper[tid & 63u] += proper;
  c->windows[tid & 63u] += windows;
}

enum AwFmReturnCode awfmPairMates(const struct AwFmPairInputs *in, uint64_t numPairs, uint32_t maxCandidates,
                                  const struct AwFmPairParams *params, const struct AwFmPairOutputs *out, unsigned threads) {
  if (numPairs == 0) return AwFmSuccess;
  if (!in || !out || !params || !in->readOffsets || !in->sequences || !in->slotScores || !in->slotReadEnds || !in->slotTextEnds)
    return AwFmNullPtrError;
  if (numPairs >= (1ull << 31) || maxCandidates < 1 || maxCandidates > AWFM_CANDIDATES_MAX_SLOTS) return AwFmIllegalPositionError;
  if (params->minInsert > params->maxInsert || params->minInsert < -AWFM_PAIR_MAX_INSERT || params->maxInsert > AWFM_PAIR_MAX_INSERT ||
      params->mapqCap > AWFM_SCORE_MAX_MAPQ)
    return AwFmIllegalPositionError;
  struct awfmPairCtx ctx;
  memset(&ctx, 0, sizeof ctx);
  ctx.in = in;
  ctx.out = out;
  ctx.params = params;
  ctx.slots = maxCandidates;
  awfmParallelFor(threads ? threads : 1, numPairs, awfmPairRange, &ctx);
  uint64_t proper = 0, windows = 0;
  for (unsigned t = 0; t < 64; t++) {
    proper += ctx.proper[t];
    windows += ctx.windows[t];
  }
  if (out->numProper) *out->numProper += proper;
  if (out->numWindows) *out->numWindows += windows;
  return AwFmSuccess;
}

struct awfmComplementCtx {
  const uint8_t *chars;
  const uint64_t *offsets;
  uint64_t numChars;
  uint32_t which;
  uint8_t *out;
  uint64_t malformed[64];
};

/* A <-> T and C <-> G in either case, the case kept; every other byte as it is */
static uint8_t awfmComplementOf(uint8_t c) {
  switch (c) {
    case 'A': return 'T';
    case 'T': return 'A';
    case 'C': return 'G';
    case 'G': return 'C';
    case 'a': return 't';
    case 't': return 'a';
    case 'c': return 'g';
    case 'g': return 'c';
    default: return c;
  }
}

static void awfmComplementRange(void *ctx, uint64_t begin, uint64_t end, unsigned tid) {
  struct awfmComplementCtx *c = ctx;
  uint64_t malformed = 0;
  for (uint64_t r = begin; r < end; r++) {
    const uint64_t readBegin = c->offsets[r], readEnd = c->offsets[r + 1u];
    if (readBegin > readEnd || readEnd > c->numChars) {
      malformed++;
      continue;
    }
    if (!c->out) continue;
    const uint64_t n = readEnd - readBegin;
    const int selected = c->which == AWFM_COMPLEMENT_ALL || (c->which == AWFM_COMPLEMENT_ODD) == (int)(r & 1u);
    for (uint64_t i = 0; i < n; i++)
      c->out[readBegin + i] = selected ? awfmComplementOf(c->chars[readBegin + n - 1u - i]) : c->chars[readBegin + i];
  }
  c->malformed[tid & 63u] += malformed;
}

enum AwFmReturnCode awfmReverseComplementReads(const uint8_t *readChars, uint64_t numReadChars, const uint64_t *readOffsets,
                                               uint64_t numReads, uint32_t which, uint8_t *out, uint64_t *numMalformed, unsigned threads) {
  if (numReads == 0) return AwFmSuccess;
  if (!readOffsets || (!readChars && numReadChars != 0)) return AwFmNullPtrError;
  if (which > AWFM_COMPLEMENT_EVEN) return AwFmIllegalPositionError;
  if (out && numReadChars && (uintptr_t)readChars < (uintptr_t)out + numReadChars && (uintptr_t)out < (uintptr_t)readChars + numReadChars)
    return AwFmIllegalPositionError;
  struct awfmComplementCtx ctx;
  memset(&ctx, 0, sizeof ctx);
  ctx.chars = readChars;
  ctx.offsets = readOffsets;
  ctx.numChars = numReadChars;
  ctx.which = which;
  ctx.out = out;
  awfmParallelFor(threads ? threads : 1, numReads, awfmComplementRange, &ctx);
  uint64_t malformed = 0;
  for (unsigned t = 0; t < 64; t++) malformed += ctx.malformed[t];
  if (numMalformed) *numMalformed += malformed;
  return AwFmSuccess;
}
