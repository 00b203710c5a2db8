/*
 * awfm_hits.h -- what the host twins of "candidate loci" and "read chains" share (awfm_candidates.c, awfm_chains.c): the
 * definition of a read's KEPT HITS (include/awfm_gpu.h, "candidate loci") -- the read's seed range and its well-formedness, the
 * walk over its kept hits with the three drop rules, the key of a diagonal, the keptHits word of a count --, the argument check
 * of the two entry points and the overflow counters of their loops.  The device's definition of the same things is
 * awfm_hits_kernel.h.  Plain C11, static inline and header-only on purpose: a twin is also compiled on its own, by naming its
 * source files.  Exact and readable rather than fast.
 */
#ifndef AWFM_HITS_H
#define AWFM_HITS_H

#include <stdint.h>

#include "awfm_gpu.h"
#include "awfm_internal.h"

#define AWFM_HITS_SIGN (1ull << 63) /* key = diagonal ^ this: unsigned order = signed order */
#define AWFM_HITS_THREADS 64u       /* overflow counters: one per thread of the loop (tid & 63) */

/* what both entry points refuse after numReads == 0, in this order: a null among the inputs (others: the call's own pointers, 0
 * when one of them is null), seeds with neither lengths nor a fixed length, more than 2^32 - 1 reads or a slot count outside
 * 1 .. 16 */
static inline enum AwFmReturnCode awfmHitsCheckArguments(const struct AwFmCandidateInputs *in, int others, uint64_t numReads,
                                                         uint32_t maxCandidates) {
  if (!in || !others || !in->readSeedOffsets || !in->seedEnds || !in->hitOffsets || !in->positions) return AwFmNullPtrError;
  if (!in->seedLengths && in->fixedLength == 0) return AwFmNullPtrError;
  if (numReads >= (1ull << 32) || maxCandidates < 1 || maxCandidates > AWFM_CANDIDATES_MAX_SLOTS) return AwFmIllegalPositionError;
  return AwFmSuccess;
}

/* read r's seeds [*seedBegin, *seedEnd); 0 for a malformed read: the range or the hit range of one of its seeds is inverted or
 * leaves its array.  Nothing is read through an offset that was not compared with its array's size first */
static inline int awfmReadSeeds(const struct AwFmCandidateInputs *in, uint64_t r, uint64_t *seedBegin, uint64_t *seedEnd) {
  const uint64_t begin = in->readSeedOffsets[r], end = in->readSeedOffsets[r + 1];
  *seedBegin = begin;
  *seedEnd = end;
  if (begin > end || end > in->numSeeds || end - begin >= (1ull << 32)) return 0;
  for (uint64_t s = begin; s < end; s++)
    if (in->hitOffsets[s] > in->hitOffsets[s + 1] || in->hitOffsets[s + 1] > in->numHits) return 0;
  return 1;
}

struct awfmKeptHit {
  uint32_t sequence, anchor, end, length; /* of the hit's seed: anchor = end - length */
  uint64_t key;                           /* the diagonal with its sign bit flipped */
};

/* where a walk over the kept hits of a well-formed read stands */
struct awfmHitCursor {
  const struct AwFmCandidateInputs *in;
  uint32_t maxHitsPerSeed, end, length;
  uint64_t seed, seedEnd, hit, hitEnd;
};

static inline struct awfmHitCursor awfmHitCursorOf(const struct AwFmCandidateInputs *in, uint32_t maxHitsPerSeed, uint64_t seedBegin,
                                                   uint64_t seedEnd) {
  const struct awfmHitCursor c = {in, maxHitsPerSeed, 0, 0, seedBegin, seedEnd, 0, 0};
  return c;
}

/* the next kept hit in the order of the arrays, 0 when there is none: seeds longer than their end and seeds of more than
 * maxHitsPerSeed hits (when that is not 0) give no hit, hits of sequence 0xFFFFFFFF are dropped */
static inline int awfmNextKeptHit(struct awfmHitCursor *c, struct awfmKeptHit *hit) {
  const struct AwFmCandidateInputs *in = c->in;
  for (;;) {
    while (c->hit == c->hitEnd) { /* the next seed that is kept */
      if (c->seed == c->seedEnd) return 0;
      const uint64_t s = c->seed++;
      c->length = in->seedLengths ? in->seedLengths[s] : in->fixedLength;
      c->end = in->seedEnds[s];
      if (c->length > c->end) continue;
      if (c->maxHitsPerSeed != 0 && in->hitOffsets[s + 1] - in->hitOffsets[s] > c->maxHitsPerSeed) continue;
      c->hit = in->hitOffsets[s];
      c->hitEnd = in->hitOffsets[s + 1];
    }
    const uint64_t h = c->hit++;
    const uint32_t sequence = in->sequenceNumbers ? in->sequenceNumbers[h] : 0;
    if (sequence == AWFM_CANDIDATES_NONE) continue;
    hit->sequence = sequence;
    hit->anchor = c->end - c->length;
    hit->end = c->end;
    hit->length = c->length;
    hit->key = (in->positions[h] - (uint64_t)hit->anchor) ^ AWFM_HITS_SIGN;
    return 1;
  }
}

/* the keptHits word of a read: kept is its true number of kept hits, or UINT64_MAX for a malformed read */
static inline uint32_t awfmKeptHitsWord(uint64_t kept) {
  return kept == UINT64_MAX ? 0xFFFFFFFFu : kept > 0xFFFFFFFEull ? 0xFFFFFFFEu : (uint32_t)kept;
}

/* the overflowed reads of a call: each thread of the loop adds to its own counter, the call adds their sum to *numOverflowed */
static inline void awfmAddOverflowed(const uint64_t counters[AWFM_HITS_THREADS], uint64_t *numOverflowed) {
  for (unsigned t = 0; numOverflowed && t < AWFM_HITS_THREADS; t++) *numOverflowed += counters[t];
}

#endif
