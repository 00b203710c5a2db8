/*
 * awfm_chains.c -- awfmReadChains (include/awfm_gpu.h, "read chains"): the best colinear chain of the kept hits of every
 * candidate slot.  The host twin of awfmGpuReadChains and its checker: one read at a time, collect the kept hits, give each to
 * the slot whose interval holds it, qsort, run the recurrence.  Nothing here is clever.  The kept hits of a read are awfm_hits.h's.
 * The reference has no analogue (it stops at positions: ref src/AwFmParallelSearch.c:315-365).
 */
#include <assert.h>
#include <stdlib.h>
#include <string.h>

#include "awfm_hits.h"

struct awfmAnchor {
  uint32_t slot, end, length;
  uint64_t key; /* the diagonal with its sign bit flipped: unsigned order = signed order */
};

/* what an anchor carries: the score of the best chain that ends in it, and that chain's first anchor */
struct awfmChainState {
  uint32_t score, anchors, begin;
  uint64_t beginKey;
};

struct awfmChainsCtx {
  const struct AwFmCandidateInputs *in;
  const struct AwFmChainOutputs *out;
  const uint32_t *sequences, *spans;
  const int64_t *diagonals;
  uint32_t maxHitsPerSeed, band, slots, lookback, gapPenalty;
  uint64_t overflowed[AWFM_HITS_THREADS];
  int failed;
};

static int awfmAnchorOrder(const void *a, const void *b) {
  const struct awfmAnchor *x = a, *y = b;
  if (x->slot != y->slot) return x->slot < y->slot ? -1 : 1;
  if (x->end != y->end) return x->end < y->end ? -1 : 1;
  if (x->key != y->key) return x->key < y->key ? -1 : 1;
  if (x->length != y->length) return x->length < y->length ? -1 : 1;
  return 0;
}

/* the last key of a slot's interval: key + span, which may pass the largest key */
static uint64_t awfmSlotHigh(uint64_t low, uint32_t span) { return low + span < low ? UINT64_MAX : low + span; }

/* two slots of the read name one sequence and their intervals intersect */
static int awfmSlotsIntersect(const struct awfmChainsCtx *c, uint64_t r) {
  for (uint32_t j = 0; j < c->slots; j++)
    for (uint32_t k = j + 1; k < c->slots; k++) {
      const uint64_t a = r * c->slots + j, b = r * c->slots + k;
      if (c->sequences[a] == AWFM_CANDIDATES_NONE || c->sequences[a] != c->sequences[b]) continue;
      const uint64_t lowA = (uint64_t)c->diagonals[a] ^ AWFM_HITS_SIGN, lowB = (uint64_t)c->diagonals[b] ^ AWFM_HITS_SIGN;
      if (lowA <= awfmSlotHigh(lowB, c->spans[b]) && lowB <= awfmSlotHigh(lowA, c->spans[a])) return 1;
    }
  return 0;
}

/* The kept hits of read r that lie in a slot, into anchors[0 .. AWFM_CANDIDATES_MAX_HITS); returns the true number of KEPT HITS
 * (in a slot or not), or UINT64_MAX for a malformed read.  *numAnchors is right when that number is within the limit. */
static uint64_t awfmCollectAnchors(const struct awfmChainsCtx *c, uint64_t r, struct awfmAnchor *anchors, size_t *numAnchors) {
  uint64_t seedBegin, seedEnd, kept = 0;
  size_t n = 0;
  *numAnchors = 0;
  if (!awfmReadSeeds(c->in, r, &seedBegin, &seedEnd) || awfmSlotsIntersect(c, r)) return UINT64_MAX;
  struct awfmHitCursor cursor = awfmHitCursorOf(c->in, c->maxHitsPerSeed, seedBegin, seedEnd);
  struct awfmKeptHit hit;
  while (awfmNextKeptHit(&cursor, &hit)) {
    if (kept++ >= AWFM_CANDIDATES_MAX_HITS) continue;
    for (uint32_t j = 0; j < c->slots; j++) {
      const uint64_t at = r * c->slots + j, low = (uint64_t)c->diagonals[at] ^ AWFM_HITS_SIGN;
      if (c->sequences[at] != hit.sequence || hit.key < low || hit.key - low > c->spans[at]) continue;
      anchors[n].slot = j;
      anchors[n].end = hit.end;
      anchors[n].length = hit.length;
      anchors[n].key = hit.key;
      n++;
      break; /* (the slots of a well-formed read do not intersect) */
    }
  }
  *numAnchors = n;
  return kept;
}

static uint64_t awfmMin3(uint64_t a, uint64_t b, uint64_t c) {
  const uint64_t ab = a < b ? a : b;
  return ab < c ? ab : c;
}

/* the recurrence over the anchors [begin, end) of one slot, in their order; returns the last anchor of the best chain */
static size_t awfmChainSlot(const struct awfmChainsCtx *c, const struct awfmAnchor *anchors, struct awfmChainState *state, size_t begin,
                            size_t end) {
  size_t best = begin;
  for (size_t i = begin; i < end; i++) {
    const struct awfmAnchor *x = &anchors[i];
    uint64_t value = 0;
    size_t from = i;
    for (size_t j = i - begin > c->lookback ? i - c->lookback : begin; j < i; j++) {
      const struct awfmAnchor *y = &anchors[j];
      if (x->end <= y->end) continue;
      const int64_t dr = (int64_t)x->end - (int64_t)y->end;
      /* both keys lie in one slot's interval: less than 2^32 apart */
      const int64_t dd = x->key >= y->key ? (int64_t)(x->key - y->key) : -(int64_t)(y->key - x->key);
      const int64_t dt = dr + dd;
      const uint64_t gap = (uint64_t)(dd < 0 ? -dd : dd);
      if (dt <= 0 || gap > c->band) continue;
      const uint64_t gain = state[j].score + awfmMin3(x->length, (uint64_t)dr, (uint64_t)dt), penalty = gap * c->gapPenalty;
      if (gain <= penalty) continue;
      if (gain - penalty >= value) { /* (ties: the largest j) */
        value = gain - penalty;
        from = j;
      }
    }
    struct awfmChainState *s = &state[i];
    if (from != i && value > x->length) {
      assert(value <= x->end); /* f(j) <= e_j and min(...) <= dr: scores fit 32 bits */
      s->score = (uint32_t)value;
      s->anchors = state[from].anchors + 1u;
      s->begin = state[from].begin;
      s->beginKey = state[from].beginKey;
    } else {
      s->score = x->length;
      s->anchors = 1u;
      s->begin = x->end - x->length;
      s->beginKey = x->key;
    }
    if (s->score > state[best].score) best = i; /* (ties: the smallest order position) */
  }
  return best;
}

static void awfmChainsRange(void *p, uint64_t begin, uint64_t end, unsigned tid) {
  struct awfmChainsCtx *c = p;
  const struct AwFmChainOutputs *out = c->out;
  struct awfmAnchor *anchors = malloc(AWFM_CANDIDATES_MAX_HITS * sizeof *anchors);
  struct awfmChainState *state = malloc(AWFM_CANDIDATES_MAX_HITS * sizeof *state);
  if (!anchors || !state) {
    c->failed = 1;
    free(anchors);
    free(state);
    return;
  }
  uint64_t overflowed = 0;
  for (uint64_t r = begin; r < end; r++) {
    size_t n = 0;
    const uint64_t kept = awfmCollectAnchors(c, r, anchors, &n);
    if (kept > AWFM_CANDIDATES_MAX_HITS) {
      overflowed++;
      n = 0;
    }
    qsort(anchors, n, sizeof *anchors, awfmAnchorOrder);
    uint32_t bestSlot = AWFM_CHAINS_NO_SLOT, bestScore = 0;
    size_t k = 0;
    for (uint32_t j = 0; j < c->slots; j++) {
      const size_t first = k;
      while (k < n && anchors[k].slot == j) k++;
      struct awfmChainState chain = {0, 0, 0, AWFM_HITS_SIGN};
      uint32_t readEnd = 0;
      uint64_t endKey = AWFM_HITS_SIGN;
      if (k > first) {
        const size_t last = awfmChainSlot(c, anchors, state, first, k);
        chain = state[last];
        readEnd = anchors[last].end;
        endKey = anchors[last].key;
        if (bestSlot == AWFM_CHAINS_NO_SLOT || chain.score > bestScore) {
          bestSlot = j;
          bestScore = chain.score;
        }
      }
      const uint64_t at = r * c->slots + j;
      if (out->chainScores) out->chainScores[at] = chain.score;
      if (out->chainAnchors) out->chainAnchors[at] = chain.anchors;
      if (out->chainReadBegins) out->chainReadBegins[at] = chain.begin;
      if (out->chainReadEnds) out->chainReadEnds[at] = readEnd;
      if (out->chainBeginDiagonals) out->chainBeginDiagonals[at] = (int64_t)(chain.beginKey ^ AWFM_HITS_SIGN);
      if (out->chainEndDiagonals) out->chainEndDiagonals[at] = (int64_t)(endKey ^ AWFM_HITS_SIGN);
    }
    if (out->bestSlots) out->bestSlots[r] = bestSlot;
    if (out->keptHits) out->keptHits[r] = awfmKeptHitsWord(kept);
  }
  free(anchors);
  free(state);
  c->overflowed[tid % AWFM_HITS_THREADS] += overflowed;
}

enum AwFmReturnCode awfmReadChains(const struct AwFmCandidateInputs *in, uint64_t numReads, uint32_t maxHitsPerSeed, uint32_t band,
                                   uint32_t maxCandidates, const uint32_t *sequences, const int64_t *diagonals,
                                   const uint32_t *diagonalSpans, uint32_t lookback, uint32_t gapPenalty,
                                   const struct AwFmChainOutputs *out, unsigned threads) {
  if (numReads == 0) return AwFmSuccess;
  const enum AwFmReturnCode refused = awfmHitsCheckArguments(in, out && sequences && diagonals && diagonalSpans, numReads, maxCandidates);
  if (refused != AwFmSuccess) return refused;
  if (lookback < 1 || lookback > AWFM_CHAINS_MAX_LOOKBACK) return AwFmIllegalPositionError;
  struct awfmChainsCtx ctx;
  memset(&ctx, 0, sizeof ctx);
  ctx.in = in;
  ctx.out = out;
  ctx.sequences = sequences;
  ctx.diagonals = diagonals;
  ctx.spans = diagonalSpans;
  ctx.maxHitsPerSeed = maxHitsPerSeed;
  ctx.band = band;
  ctx.slots = maxCandidates;
  ctx.lookback = lookback;
  ctx.gapPenalty = gapPenalty;
  awfmParallelFor(threads ? threads : 1, numReads, awfmChainsRange, &ctx);
  if (ctx.failed) return AwFmAllocationFailure;
  awfmAddOverflowed(ctx.overflowed, out->numOverflowed);
  return AwFmSuccess;
}
