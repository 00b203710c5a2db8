/*
 * awfm_candidates.c -- awfmReadCandidates (include/awfm_gpu.h, "candidate loci"): the located seeds of a read grouped into
 * clusters of (sequence, diagonal), the best few kept.  The host twin of awfmGpuReadCandidates and its checker: one read at a
 * time, collect the kept hits, qsort, scan the runs, select.  Nothing here is clever.  The reference has no analogue (it stops
 * at positions: ref src/AwFmParallelSearch.c:315-365).
 */
#include <stdlib.h>
#include <string.h>

#include "awfm_hits.h"

struct awfmCluster {
  uint32_t sequence, votes, span, begin, end;
  uint64_t key;
};

struct awfmCandidatesCtx {
  const struct AwFmCandidateInputs *in;
  const struct AwFmCandidateOutputs *out;
  uint32_t maxHitsPerSeed, band, minVotes, slots;
  uint64_t overflowed[AWFM_HITS_THREADS];
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

/* the kept hits of read r (awfm_hits.h) into hits[0 .. AWFM_CANDIDATES_MAX_HITS); returns their true number, or UINT64_MAX for
 * a malformed read */
static uint64_t awfmCollectKeptHits(const struct awfmCandidatesCtx *c, uint64_t r, struct awfmKeptHit *hits) {
  uint64_t seedBegin, seedEnd, kept = 0;
  if (!awfmReadSeeds(c->in, r, &seedBegin, &seedEnd)) return UINT64_MAX;
  struct awfmHitCursor cursor = awfmHitCursorOf(c->in, c->maxHitsPerSeed, seedBegin, seedEnd);
  struct awfmKeptHit hit;
  while (awfmNextKeptHit(&cursor, &hit)) {
    if (kept < AWFM_CANDIDATES_MAX_HITS) hits[kept] = hit;
    kept++;
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
    if (out->keptHits) out->keptHits[r] = awfmKeptHitsWord(kept);
    size_t last = 0; /* slot j: the best candidate after slot j - 1's */
    for (uint32_t j = 0; j < c->slots; j++) {
      size_t best = numClusters;
      if (j < numCandidates)
        for (size_t k = 0; k < numClusters; k++) {
          if (clusters[k].votes < c->minVotes) continue;
          if (j != 0 && !awfmClusterBefore(&clusters[last], last, &clusters[k], k)) continue;
          if (best == numClusters || awfmClusterBefore(&clusters[k], k, &clusters[best], best)) best = k;
        }
      const struct awfmCluster none = {AWFM_CANDIDATES_NONE, 0, 0, 0, 0, AWFM_HITS_SIGN};
      const struct awfmCluster *cl = best < numClusters ? &clusters[best] : &none;
      const uint64_t at = r * c->slots + j;
      if (out->sequences) out->sequences[at] = cl->sequence;
      if (out->diagonals) out->diagonals[at] = (int64_t)(cl->key ^ AWFM_HITS_SIGN);
      if (out->votes) out->votes[at] = cl->votes;
      if (out->diagonalSpans) out->diagonalSpans[at] = cl->span;
      if (out->readBegins) out->readBegins[at] = cl->begin;
      if (out->readEnds) out->readEnds[at] = cl->end;
      last = best;
    }
  }
  free(hits);
  free(clusters);
  c->overflowed[tid % AWFM_HITS_THREADS] += overflowed;
}

enum AwFmReturnCode awfmReadCandidates(const struct AwFmCandidateInputs *in, uint64_t numReads, uint32_t maxHitsPerSeed, uint32_t band,
                                       uint32_t minVotes, uint32_t maxCandidates, const struct AwFmCandidateOutputs *out,
                                       unsigned threads) {
  if (numReads == 0) return AwFmSuccess;
  const enum AwFmReturnCode refused = awfmHitsCheckArguments(in, out != NULL, numReads, maxCandidates);
  if (refused != AwFmSuccess) return refused;
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
  awfmAddOverflowed(ctx.overflowed, out->numOverflowed);
  return AwFmSuccess;
}
