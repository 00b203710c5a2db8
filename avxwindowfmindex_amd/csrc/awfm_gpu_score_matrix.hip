/*
 * awfm_gpu_score_matrix.hip -- "substitution matrices" on the device (include/awfm_gpu.h): awfmGpuScoreChainsMatrix, slot scores
 * with the diagonal's score from the caller's matrix.  The kernel is awfm_matrix_kernel.h, the host twin and checker
 * awfmScoreChainsMatrix (awfm_score_affine.c); the checks, the parameters and the grid are awfmGpuScoreChainsAffine's
 * (scoreChainsArgumentsRefused, scoreChainsParams).  One launch, no scratch; the matrix goes into the launch's arguments by value.
 */
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <shared_mutex>

#include "awfm_matrix_kernel.h"

extern "C" {

enum AwFmReturnCode awfmGpuScoreChainsMatrix(AwFmGpuIndex *g, const struct AwFmVerifyInputs *dIn, uint64_t numReads, uint32_t maxCandidates,
                                             uint32_t bandPad, uint32_t maxDrift, const struct AwFmMatrixScoring *scoring, uint32_t minScore,
                                             uint32_t mapqCap, const struct AwFmSlotScoreOutputs *dOut, void *stream) {
  if (!g) {
    setError("awfmGpuScoreChainsMatrix: null image");
    return AwFmNullPtrError;
  }
  if (numReads == 0) return AwFmSuccess;
  const char *name = "awfmGpuScoreChainsMatrix";
  enum AwFmReturnCode rc = scoreChainsArgumentsRefused(
      name, dIn, scoring, [&] { return matrixScoringRefused(name, scoring); }, numReads, maxCandidates, bandPad, maxDrift, mapqCap, dOut);
  if (rc != AwFmSuccess) return rc;
  DeviceGuard guard(g->device);
  AwFmGpuImage *image = g->image;
  std::shared_lock<std::shared_mutex> lock(image->recordMutex); /* neither text nor record table is replaced before the launch */
  if ((rc = textMissing(name, image)) != AwFmSuccess) return rc;
  DevScoreMatrixParams p{};
  unsigned group;
  dim3 grid;
  const dim3 block(kScoreThreads);
  scoreChainsParams(g, dIn, numReads, maxCandidates, bandPad, maxDrift, minScore, mapqCap, dOut, p, group, grid);
  p.open = (int)(scoring->gapOpen + scoring->gapExtend);
  p.extend = (int)scoring->gapExtend;
  memcpy(p.matrix, scoring->substitution, sizeof p.matrix);
  AWFM_LAUNCH_BAND_KERNEL(scoreChainsMatrixKernel, group, grid, block, stream, p);
  AWFM_HIP_TRY(hipGetLastError(), AwFmGeneralFailure);
  return AwFmSuccess;
}

}  // extern "C"
