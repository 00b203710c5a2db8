/*
 * awfm_gpu_align_affine.hip -- "affine alignment" on the device (include/awfm_gpu.h): awfmGpuAlignChainsAffine and the size of its
 * trace arena.  The kernel is awfm_align_affine_kernel.h, the host twin and checker awfm_align_affine.c.
 */
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <shared_mutex>

#include "awfm_align_affine_kernel.h"

extern "C" {

uint64_t awfmGpuAlignChainsAffineScratchBytes(const AwFmGpuIndex *g, uint32_t maxRows) {
  if (!g || maxRows < 1 || maxRows > AWFM_ALIGN_MAX_LENGTH) return 0;
  return affineGridWaves(g) * kAffineRowBytes * maxRows;
}

enum AwFmReturnCode awfmGpuAlignChainsAffine(AwFmGpuIndex *g, const struct AwFmVerifyInputs *dIn, const uint32_t *dSlots, uint64_t numReads,
                                             uint32_t maxCandidates, uint32_t bandPad, uint32_t maxDrift,
                                             const struct AwFmAlignScoring *scoring, uint32_t maxOps, uint32_t maxRows,
                                             const struct AwFmAffineOutputs *dOut, void *dScratch, void *stream) {
  if (!g) {
    setError("awfmGpuAlignChainsAffine: null image");
    return AwFmNullPtrError;
  }
  if (numReads == 0) return AwFmSuccess;
  const char *name = "awfmGpuAlignChainsAffine";
  enum AwFmReturnCode rc = alignChainsArgumentsRefused(
      name, dIn, dSlots, scoring, [&] { return scoringRefused(name, scoring); }, numReads, maxCandidates, bandPad, maxDrift, maxOps, maxRows, dOut,
      dScratch);
  if (rc != AwFmSuccess) return rc;
  DeviceGuard guard(g->device);
  AwFmGpuImage *image = g->image;
  std::shared_lock<std::shared_mutex> lock(image->recordMutex); /* neither text nor record table is replaced before the launch */
  if ((rc = textMissing(name, image)) != AwFmSuccess) return rc;
  DevAffineParams p{};
  unsigned group;
  dim3 grid;
  const dim3 block(kAffineThreads);
  alignChainsParams(g, dIn, dSlots, numReads, maxCandidates, bandPad, maxDrift, maxOps, maxRows, dOut, dScratch, p, group, grid);
  p.match = (int)scoring->match;
  p.mismatch = (int)scoring->mismatch;
  p.open = (int)(scoring->gapOpen + scoring->gapExtend);
  p.extend = (int)scoring->gapExtend;
  AWFM_LAUNCH_BAND_KERNEL(alignChainsAffineKernel, group, grid, block, stream, p);
  AWFM_HIP_TRY(hipGetLastError(), AwFmGeneralFailure);
  return AwFmSuccess;
}

}  // extern "C"
