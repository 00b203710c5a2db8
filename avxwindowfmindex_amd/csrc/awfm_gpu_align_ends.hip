/*
 * awfm_gpu_align_ends.hip -- "end bonus" on the device (include/awfm_gpu.h): awfmGpuAlignChainsEndBonus, affine alignment under a
 * substitution matrix with B for a read end that is reached.  The kernel is awfm_end_bonus_kernel.h, the host twin and checker
 * awfmAlignChainsEndBonus (awfm_align_affine.c); the checks, the parameters, the grid and the trace arena are
 * awfmGpuAlignChainsAffine's (alignChainsArgumentsRefused, alignChainsParams).  The matrix and B go into the launch's arguments
 * by value.
 */
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <shared_mutex>

#include "awfm_end_bonus_kernel.h"

extern "C" {

enum AwFmReturnCode awfmGpuAlignChainsEndBonus(AwFmGpuIndex *g, const struct AwFmVerifyInputs *dIn, const uint32_t *dSlots, uint64_t numReads,
                                               uint32_t maxCandidates, uint32_t bandPad, uint32_t maxDrift,
                                               const struct AwFmMatrixScoring *scoring, uint32_t endBonus, uint32_t maxOps, uint32_t maxRows,
                                               const struct AwFmAffineOutputs *dOut, void *dScratch, void *stream) {
  if (!g) {
    setError("awfmGpuAlignChainsEndBonus: null image");
    return AwFmNullPtrError;
  }
  if (numReads == 0) return AwFmSuccess;
  const char *name = "awfmGpuAlignChainsEndBonus";
  enum AwFmReturnCode rc = alignChainsArgumentsRefused(
      name, dIn, dSlots, scoring, [&] { return endBonusScoringRefused(name, scoring, endBonus); }, numReads, maxCandidates, bandPad, maxDrift,
      maxOps, maxRows, dOut, dScratch);
  if (rc != AwFmSuccess) return rc;
  DeviceGuard guard(g->device);
  AwFmGpuImage *image = g->image;
  std::shared_lock<std::shared_mutex> lock(image->recordMutex); /* neither text nor record table is replaced before the launch */
  if ((rc = textMissing(name, image)) != AwFmSuccess) return rc;
  DevAffineEndBonusParams p{};
  unsigned group;
  dim3 grid;
  const dim3 block(kAffineThreads);
  alignChainsParams(g, dIn, dSlots, numReads, maxCandidates, bandPad, maxDrift, maxOps, maxRows, dOut, dScratch, p, group, grid);
  p.open = (int)(scoring->gapOpen + scoring->gapExtend);
  p.extend = (int)scoring->gapExtend;
  memcpy(p.matrix, scoring->substitution, sizeof p.matrix);
  p.endBonus = endBonus;
  AWFM_LAUNCH_BAND_KERNEL(alignChainsEndBonusKernel, group, grid, block, stream, p);
  AWFM_HIP_TRY(hipGetLastError(), AwFmGeneralFailure);
  return AwFmSuccess;
}

}  // extern "C"
