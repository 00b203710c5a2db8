/*
 * awfm_gpu_score_ends.hip -- "end bonus" on the device (include/awfm_gpu.h): awfmGpuScoreChainsEndBonus, slot scores under a
 * substitution matrix with B for a read end that is reached.  The kernel is awfm_end_bonus_kernel.h, the host twin and checker
 * awfmScoreChainsEndBonus (awfm_score_affine.c); the checks, the parameters and the grid are awfmGpuScoreChainsAffine's
 * (scoreChainsArgumentsRefused, scoreChainsParams).  One launch, no scratch; the matrix and B go into the launch's arguments by
 * value.
 */
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <shared_mutex>

#include "awfm_end_bonus_kernel.h"

extern "C" {

enum AwFmReturnCode awfmGpuScoreChainsEndBonus(AwFmGpuIndex *g, const struct AwFmVerifyInputs *dIn, uint64_t numReads, uint32_t maxCandidates,
                                               uint32_t bandPad, uint32_t maxDrift, const struct AwFmMatrixScoring *scoring, uint32_t endBonus,
                                               uint32_t minScore, uint32_t mapqCap, const struct AwFmSlotScoreOutputs *dOut, void *stream) {
  if (!g) {
    setError("awfmGpuScoreChainsEndBonus: null image");
    return AwFmNullPtrError;
  }
  if (numReads == 0) return AwFmSuccess;
  const char *name = "awfmGpuScoreChainsEndBonus";
  enum AwFmReturnCode rc = scoreChainsArgumentsRefused(
      name, dIn, scoring, [&] { return endBonusScoringRefused(name, scoring, endBonus); }, numReads, maxCandidates, bandPad, maxDrift, mapqCap,
      dOut);
  if (rc != AwFmSuccess) return rc;
  DeviceGuard guard(g->device);
  AwFmGpuImage *image = g->image;
  std::shared_lock<std::shared_mutex> lock(image->recordMutex); /* neither text nor record table is replaced before the launch */
  if ((rc = textMissing(name, image)) != AwFmSuccess) return rc;
  DevScoreEndBonusParams p{};
  unsigned group;
  dim3 grid;
  const dim3 block(kScoreThreads);
  scoreChainsParams(g, dIn, numReads, maxCandidates, bandPad, maxDrift, minScore, mapqCap, dOut, p, group, grid);
  p.open = (int)(scoring->gapOpen + scoring->gapExtend);
  p.extend = (int)scoring->gapExtend;
  memcpy(p.matrix, scoring->substitution, sizeof p.matrix);
  p.endBonus = endBonus;
  AWFM_LAUNCH_BAND_KERNEL(scoreChainsEndBonusKernel, group, grid, block, stream, p);
  AWFM_HIP_TRY(hipGetLastError(), AwFmGeneralFailure);
  return AwFmSuccess;
}

}  // extern "C"
