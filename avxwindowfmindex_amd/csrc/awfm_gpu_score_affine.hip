/*
 * awfm_gpu_score_affine.hip -- "slot scores and mapping quality" on the device (include/awfm_gpu.h): awfmGpuScoreChainsAffine.  The
 * kernel is awfm_score_affine_kernel.h, the host twin and checker awfm_score_affine.c.  One launch, no scratch, none of the
 * handle's scratch slots.
 */
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <shared_mutex>

#include "awfm_score_affine_kernel.h"

extern "C" {

enum AwFmReturnCode awfmGpuScoreChainsAffine(AwFmGpuIndex *g, const struct AwFmVerifyInputs *dIn, uint64_t numReads, uint32_t maxCandidates,
                                             uint32_t bandPad, uint32_t maxDrift, const struct AwFmAlignScoring *scoring, uint32_t minScore,
                                             uint32_t mapqCap, const struct AwFmSlotScoreOutputs *dOut, void *stream) {
  if (!g) {
    setError("awfmGpuScoreChainsAffine: null image");
    return AwFmNullPtrError;
  }
  if (numReads == 0) return AwFmSuccess;
  const char *name = "awfmGpuScoreChainsAffine";
  const uint64_t band = (uint64_t)maxDrift + 2ull * bandPad + 1ull;
  enum AwFmReturnCode rc = chainArgumentsRefused(name, dIn, dOut && scoring, numReads, maxCandidates, band);
  if (rc != AwFmSuccess) return rc;
  if (mapqCap > AWFM_SCORE_MAX_MAPQ) {
    setCallError(name, "mapqCap is 0 to 254");
    return AwFmIllegalPositionError;
  }
  if ((rc = scoringRefused(name, scoring)) != AwFmSuccess) return rc;
  DeviceGuard guard(g->device);
  AwFmGpuImage *image = g->image;
  std::shared_lock<std::shared_mutex> lock(image->recordMutex); /* neither text nor record table is replaced before the launch */
  if ((rc = textMissing(name, image)) != AwFmSuccess) return rc;
  DevScoreParams p{};
  p.in = *dIn;
  p.out = *dOut;
  p.text = (const unsigned char *)image->dText;
  p.length = image->textLength;
  p.ends = image->records.ends;
  p.numRecords = image->records.numRecords;
  p.numReads = numReads;
  p.slots = maxCandidates;
  p.pad = bandPad;
  p.drift = maxDrift;
  p.amino = g->amino ? 1u : 0u;
  p.floor = minScore > 1u ? minScore : 1u;
  p.cap = mapqCap;
  p.match = (int)scoring->match;
  p.mismatch = (int)scoring->mismatch;
  p.open = (int)(scoring->gapOpen + scoring->gapExtend);
  p.extend = (int)scoring->gapExtend;
  const unsigned group = bandGroup(band, "score_group");
  /* persistent grid over reads, a wave each */
  const uint64_t perBlock = kScoreThreads / 64u, blocks = (numReads + perBlock - 1u) / perBlock;
  const uint64_t resident = (uint64_t)g->numCUs * kScoreBlocksPerCU;
  const dim3 grid((unsigned)(blocks < resident ? blocks : resident)), block(kScoreThreads);
  AWFM_LAUNCH_BAND_KERNEL(scoreChainsAffineKernel, group, grid, block, stream, p);
  AWFM_HIP_TRY(hipGetLastError(), AwFmGeneralFailure);
  return AwFmSuccess;
}

}  // extern "C"
