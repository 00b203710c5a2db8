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
  enum AwFmReturnCode rc = scoreChainsArgumentsRefused(
      name, dIn, scoring, [&] { return scoringRefused(name, scoring); }, numReads, maxCandidates, bandPad, maxDrift, mapqCap, dOut);
  if (rc != AwFmSuccess) return rc;
  DeviceGuard guard(g->device);
  AwFmGpuImage *image = g->image;
  std::shared_lock<std::shared_mutex> lock(image->recordMutex); /* neither text nor record table is replaced before the launch */
  if ((rc = textMissing(name, image)) != AwFmSuccess) return rc;
  DevScoreParams p{};
  unsigned group;
  dim3 grid;
  const dim3 block(kScoreThreads);
  scoreChainsParams(g, dIn, numReads, maxCandidates, bandPad, maxDrift, minScore, mapqCap, dOut, p, group, grid);
  p.match = (int)scoring->match;
  p.mismatch = (int)scoring->mismatch;
  p.open = (int)(scoring->gapOpen + scoring->gapExtend);
  p.extend = (int)scoring->gapExtend;
  AWFM_LAUNCH_BAND_KERNEL(scoreChainsAffineKernel, group, grid, block, stream, p);
  AWFM_HIP_TRY(hipGetLastError(), AwFmGeneralFailure);
  return AwFmSuccess;
}

}  // extern "C"
