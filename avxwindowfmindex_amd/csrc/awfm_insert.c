/*
 * awfm_insert.c -- awfmInsertHistogram and awfmInsertInterval (include/awfm_gpu.h, "insert size"): the histogram of the template
 * lengths of the pairs whose two best slots agree, and the insert interval from its quartiles.  The host twins of
 * awfmGpuInsertHistogram and awfmGpuInsertInterval and their checkers: a pair at a time, a bin at a time, the header's rules as
 * written, integers only.  Exact and readable rather than fast.  The reference has no analogue (it stops at positions:
 * ref src/AwFmParallelSearch.c:315-365).
 */
#include <stdlib.h>
#include <string.h>

#include "awfm_gpu.h"
#include "awfm_internal.h"

/* what all four calls of the section ask of their params */
static int awfmInsertParamsAreLegal(const struct AwFmInsertParams *q) {
  if (q->lowTemplate > q->highTemplate || q->lowTemplate < -AWFM_PAIR_MAX_INSERT || q->highTemplate > AWFM_PAIR_MAX_INSERT) return 0;
  if ((uint64_t)(q->highTemplate - q->lowTemplate) >= AWFM_INSERT_MAX_BINS) return 0;
  if (q->spread > AWFM_INSERT_MAX_SPREAD) return 0;
  return q->fallbackMin <= q->fallbackMax && q->fallbackMin >= -AWFM_PAIR_MAX_INSERT && q->fallbackMax <= AWFM_PAIR_MAX_INSERT;
}

struct awfmInsertCtx {
  const struct AwFmPairInputs *in;
  const struct AwFmInsertParams *params;
  uint32_t slots;
  uint64_t *histogram;
  uint64_t samples[64], outside[64]; /* per thread of the loop */
};

static void awfmInsertRange(void *ctx, uint64_t begin, uint64_t end, unsigned tid) {
  struct awfmInsertCtx *c = ctx;
  const struct AwFmPairInputs *in = c->in;
  const struct AwFmInsertParams *q = c->params;
  const uint32_t C = c->slots, floor = q->minScore > 1u ? q->minScore : 1u;
  uint64_t samples = 0, outside = 0;
  for (uint64_t p = begin; p < end; p++) {
    /* pairing's rules 1 and 2: each mate's best slot, the largest score that counts, ties to the lowest slot */
    uint32_t best[2];
    int64_t start[2];
    int qualifies = 1;
    for (int m = 0; m < 2; m++) {
      const uint64_t r = 2u * p + (uint64_t)m, readBegin = in->readOffsets[r], readEnd = in->readOffsets[r + 1u];
      best[m] = AWFM_CHAINS_NO_SLOT;
      for (uint32_t j = 0; j < C; j++) {
        const uint32_t score = in->slotScores[r * C + j];
        const int counts = readBegin <= readEnd && score < AWFM_VERIFY_TOO_LONG && score >= floor;
        if (counts && (best[m] == AWFM_CHAINS_NO_SLOT || score > in->slotScores[r * C + best[m]])) best[m] = j;
      }
      if (best[m] == AWFM_CHAINS_NO_SLOT) {
        qualifies = 0;
        break;
      }
      start[m] = (int64_t)(in->slotTextEnds[r * C + best[m]] - (uint64_t)in->slotReadEnds[r * C + best[m]]);
      const uint32_t given = in->mappingQualities ? in->mappingQualities[r] : 0u;
      if (given < q->minQuality) qualifies = 0;
    }
    if (!qualifies) continue;
    const uint64_t A = 2u * p, B = A + 1u;
    if (in->sequences[A * C + best[0]] != in->sequences[B * C + best[1]]) continue;
    const uint64_t nB = in->readOffsets[B + 1u] - in->readOffsets[B];
    const int64_t T = (int64_t)((uint64_t)start[1] + nB - (uint64_t)start[0]);
    if (q->lowTemplate <= T && T <= q->highTemplate) {
      __atomic_fetch_add(&c->histogram[T - q->lowTemplate], 1u, __ATOMIC_RELAXED);
      samples++;
    } else {
      outside++;
    }
  }
  c->samples[tid & 63u] += samples;
  c->outside[tid & 63u] += outside;
}

enum AwFmReturnCode awfmInsertHistogram(const struct AwFmPairInputs *in, uint64_t numPairs, uint32_t maxCandidates,
                                        const struct AwFmInsertParams *params, uint64_t *histogram, uint64_t *numSamples,
                                        uint64_t *numOutside, unsigned threads) {
  if (numPairs == 0) return AwFmSuccess;
  if (!in || !params || !histogram || !in->readOffsets || !in->sequences || !in->slotScores || !in->slotReadEnds || !in->slotTextEnds)
    return AwFmNullPtrError;
  if (numPairs >= (1ull << 31) || maxCandidates < 1 || maxCandidates > AWFM_CANDIDATES_MAX_SLOTS) return AwFmIllegalPositionError;
  if (!awfmInsertParamsAreLegal(params)) return AwFmIllegalPositionError;
  struct awfmInsertCtx ctx;
  memset(&ctx, 0, sizeof ctx);
  ctx.in = in;
  ctx.params = params;
  ctx.slots = maxCandidates;
  ctx.histogram = histogram;
  awfmParallelFor(threads ? threads : 1, numPairs, awfmInsertRange, &ctx);
  uint64_t samples = 0, outside = 0;
  for (unsigned t = 0; t < 64; t++) {
    samples += ctx.samples[t];
    outside += ctx.outside[t];
  }
  if (numSamples) *numSamples += samples;
  if (numOutside) *numOutside += outside;
  return AwFmSuccess;
}

static int64_t awfmInsertClamped(int64_t x) {
  return x < -AWFM_PAIR_MAX_INSERT ? -AWFM_PAIR_MAX_INSERT : x > AWFM_PAIR_MAX_INSERT ? AWFM_PAIR_MAX_INSERT : x;
}

enum AwFmReturnCode awfmInsertInterval(const uint64_t *histogram, const struct AwFmInsertParams *params, struct AwFmInsertEstimate *estimate) {
  if (!histogram || !params || !estimate) return AwFmNullPtrError;
  if (!awfmInsertParamsAreLegal(params)) return AwFmIllegalPositionError;
  const uint64_t bins = (uint64_t)(params->highTemplate - params->lowTemplate) + 1u;
  uint64_t N = 0;
  for (uint64_t i = 0; i < bins; i++) N += histogram[i];
  struct AwFmInsertEstimate e;
  memset(&e, 0, sizeof e);
  e.numSamples = N;
  if (N < (params->minSamples > 1u ? params->minSamples : 1u)) {
    e.minInsert = params->fallbackMin;
    e.maxInsert = params->fallbackMax;
    *estimate = e;
    return AwFmSuccess;
  }
  /* the three quartiles in one pass: q_k is the first bin whose inclusive prefix sum reaches rank_k */
  uint64_t prefix = 0;
  unsigned k = 1;
  for (uint64_t i = 0; i < bins && k <= 3u; i++) {
    prefix += histogram[i];
    while (k <= 3u && prefix >= ((uint64_t)k * N + 3u) / 4u) e.quartiles[k++ - 1u] = params->lowTemplate + (int64_t)i;
  }
  const int64_t range = e.quartiles[2] - e.quartiles[0], w = (int64_t)params->spread * (range > 1 ? range : 1);
  e.minInsert = awfmInsertClamped(e.quartiles[0] - w);
  e.maxInsert = awfmInsertClamped(e.quartiles[2] + w);
  uint64_t weighted = 0, inliers = 0;
  for (uint64_t i = 0; i < bins; i++) {
    const int64_t T = params->lowTemplate + (int64_t)i;
    if (T < e.minInsert || T > e.maxInsert) continue;
    weighted += i * histogram[i];
    inliers += histogram[i];
  }
  e.mean = params->lowTemplate + (int64_t)(weighted / inliers);
  e.valid = 1;
  *estimate = e;
  return AwFmSuccess;
}
