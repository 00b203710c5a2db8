/*
 * awfm_candidates.c -- awfmReadCandidates (include/awfm_gpu.h, "candidate loci"): the located seeds of a read grouped into
 * clusters of (sequence, diagonal), the best few kept.  The host twin of awfmGpuReadCandidates and its checker: one read at a
 * time, collect the kept hits, qsort, scan the runs, select.  Nothing here is clever.  The reference has no analogue (it stops
 * at positions: ref src/AwFmParallelSearch.c:315-365).
 */
#include <stdlib.h>
#include <string.h>

#include "awfm_gpu.h"
#include "awfm_internal.h"

struct awfmKeptHit {
  uint32_t sequence;
  uint64_t key; /* the diagonal with its sign bit flipped: unsigned order = signed order */
  uint32_t anchor, end;
};

struct awfmCluster {
  uint32_t sequence, votes, span, begin, end;
  uint64_t key;
};

struct awfmCandidatesCtx {
  const struct AwFmCandidateInputs *in;
  const struct AwFmCandidateOutputs *out;
  uint32_t maxHitsPerSeed, band, minVotes, slots;
  uint64_t overflowed[64]; /* per thread of the loop */
  int failed;
};

static int awfmKeptHitOrder(const void *a, const void *b) {
  const struct awfmKeptHit *x = a, *y = b;
  if (x->sequence != y->sequence) return x->sequence < y->sequence ? -1 : 1;
  if (x->key != y->key) return x->key < y->key ? -1 : 1;
  return 0;
}

/* (votes descending; the clusters are made in (sequence, diagonal) order, so their number breaks ties) */
static int awfmClusterBefore(const struct awfmCluster *x, size_t xAt, const struct awfmCluster *y, size_t yAt) {
  return x->votes != y->votes ? x->votes > y->votes : xAt < yAt;
}

/* the kept hits of read r into hits[0 .. AWFM_CANDIDATES_MAX_HITS); returns their true number, or UINT64_MAX for a malformed read */
static uint64_t awfmCollectKeptHits(const struct awfmCandidatesCtx *c, uint64_t r, struct awfmKeptHit *hits) {
  const struct AwFmCandidateInputs *in = c->in;
  const uint64_t seedBegin = in->readSeedOffsets[r], seedEnd = in->readSeedOffsets[r + 1];
  if (seedBegin > seedEnd || seedEnd > in->numSeeds || seedEnd - seedBegin >= (1ull << 32)) return UINT64_MAX;
  for (uint64_t s = seedBegin; s < seedEnd; s++)
    if (in->hitOffsets[s] > in->hitOffsets[s + 1] || in->hitOffsets[s + 1] > in->numHits) return UINT64_MAX;
  uint64_t kept = 0;
  for (uint64_t s = seedBegin; s < seedEnd; s++) {
    const uint32_t length = in->seedLengths ? in->seedLengths[s] : in->fixedLength, end = in->seedEnds[s];
    const uint64_t hitBegin = in->hitOffsets[s], hitEnd = in->hitOffsets[s + 1];
    if (length > end) continue;
    if (c->maxHitsPerSeed != 0 && hitEnd - hitBegin > c->maxHitsPerSeed) continue;
    for (uint64_t h = hitBegin; h < hitEnd; h++) {
      const uint32_t sequence = in->sequenceNumbers ? in->sequenceNumbers[h] : 0;
      if (sequence == AWFM_CANDIDATES_NONE) continue;
      if (kept < AWFM_CANDIDATES_MAX_HITS) {
        struct awfmKeptHit *hit = &hits[kept];
        hit->sequence = sequence;
        hit->key = (in->positions[h] - (uint64_t)(end - length)) ^ (1ull << 63);
        hit->anchor = end - length;
        hit->end = end;
      }
      kept++;
    }
  }
  return kept;
}

static void awfmCandidatesRange(void *p, uint64_t begin, uint64_t end, unsigned tid) {
  struct awfmCandidatesCtx *c = p;
  const struct AwFmCandidateOutputs *out = c->out;
  struct awfmKeptHit *hits = malloc(AWFM_CANDIDATES_MAX_HITS * sizeof *hits);
  struct awfmCluster *clusters = malloc(AWFM_CANDIDATES_MAX_HITS * sizeof *clusters);
  if (!hits || !clusters) {
    c->failed = 1;
    free(hits);
    free(clusters);
    return;
  }
  uint64_t overflowed = 0;
  for (uint64_t r = begin; r < end; r++) {
    const uint64_t kept = awfmCollectKeptHits(c, r, hits);
    size_t numClusters = 0, numCandidates = 0;
    if (kept > AWFM_CANDIDATES_MAX_HITS)
      overflowed++;
    else {
      qsort(hits, kept, sizeof *hits, awfmKeptHitOrder);
      for (size_t k = 0; k < kept; k++) {
        const struct awfmKeptHit *hit = &hits[k];
        struct awfmCluster *cl = numClusters ? &clusters[numClusters - 1] : NULL;
        if (k == 0 || hit->sequence != hits[k - 1].sequence || hit->key - hits[k - 1].key > c->band) {
          cl = &clusters[numClusters++];
          cl->sequence = hit->sequence;
          cl->key = hit->key;
          cl->votes = 0;
          cl->begin = hit->anchor;
          cl->end = hit->end;
        }
        cl->votes++;
        cl->span = hit->key - cl->key > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)(hit->key - cl->key);
        if (hit->anchor < cl->begin) cl->begin = hit->anchor;
        if (hit->end > cl->end) cl->end = hit->end;
      }
      for (size_t k = 0; k < numClusters; k++) numCandidates += clusters[k].votes >= c->minVotes;
    }
    if (out->numCandidates) out->numCandidates[r] = (uint32_t)numCandidates;
    if (out->keptHits) out->keptHits[r] = kept == UINT64_MAX ? 0xFFFFFFFFu : kept > 0xFFFFFFFEull ? 0xFFFFFFFEu : (uint32_t)kept;
    size_t last = 0; /* slot j: the best candidate after slot j - 1's */
    for (uint32_t j = 0; j < c->slots; j++) {
      size_t best = numClusters;
      if (j < numCandidates)
        for (size_t k = 0; k < numClusters; k++) {
          if (clusters[k].votes < c->minVotes) continue;
          if (j != 0 && !awfmClusterBefore(&clusters[last], last, &clusters[k], k)) continue;
          if (best == numClusters || awfmClusterBefore(&clusters[k], k, &clusters[best], best)) best = k;
        }
      const struct awfmCluster none = {AWFM_CANDIDATES_NONE, 0, 0, 0, 0, 1ull << 63};
      const struct awfmCluster *cl = best < numClusters ? &clusters[best] : &none;
      const uint64_t at = r * c->slots + j;
      if (out->sequences) out->sequences[at] = cl->sequence;
      if (out->diagonals) out->diagonals[at] = (int64_t)(cl->key ^ (1ull << 63));
      if (out->votes) out->votes[at] = cl->votes;
      if (out->diagonalSpans) out->diagonalSpans[at] = cl->span;
      if (out->readBegins) out->readBegins[at] = cl->begin;
      if (out->readEnds) out->readEnds[at] = cl->end;
      last = best;
    }
  }
  free(hits);
  free(clusters);
  c->overflowed[tid & 63u] += overflowed;
}

enum AwFmReturnCode awfmReadCandidates(const struct AwFmCandidateInputs *in, uint64_t numReads, uint32_t maxHitsPerSeed, uint32_t band,
                                       uint32_t minVotes, uint32_t maxCandidates, const struct AwFmCandidateOutputs *out,
                                       unsigned threads) {
  if (numReads == 0) return AwFmSuccess;
  if (!in || !out || !in->readSeedOffsets || !in->seedEnds || !in->hitOffsets || !in->positions) return AwFmNullPtrError;
  if (!in->seedLengths && in->fixedLength == 0) return AwFmNullPtrError;
  if (numReads >= (1ull << 32) || maxCandidates < 1 || maxCandidates > AWFM_CANDIDATES_MAX_SLOTS) return AwFmIllegalPositionError;
  struct awfmCandidatesCtx ctx;
  memset(&ctx, 0, sizeof ctx);
  ctx.in = in;
  ctx.out = out;
  ctx.maxHitsPerSeed = maxHitsPerSeed;
  ctx.band = band;
  ctx.minVotes = minVotes ? minVotes : 1;
  ctx.slots = maxCandidates;
  awfmParallelFor(threads ? threads : 1, numReads, awfmCandidatesRange, &ctx);
  if (ctx.failed) return AwFmAllocationFailure;
  uint64_t overflowed = 0;
  for (unsigned t = 0; t < 64; t++) overflowed += ctx.overflowed[t];
  if (out->numOverflowed) *out->numOverflowed += overflowed;
  return AwFmSuccess;
}
