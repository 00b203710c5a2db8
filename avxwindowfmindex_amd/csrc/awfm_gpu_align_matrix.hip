/*
 * awfm_gpu_align_matrix.hip -- "substitution matrices" on the device (include/awfm_gpu.h): awfmGpuAlignChainsMatrix, affine
 * alignment with the diagonal's score from the caller's matrix.  The kernel is awfm_matrix_kernel.h, the host twin and checker
 * awfmAlignChainsMatrix (awfm_align_affine.c); the checks, the parameters, the grid and the trace arena are
 * awfmGpuAlignChainsAffine's (alignChainsArgumentsRefused, alignChainsParams).  The matrix goes into the launch's arguments by value.
 */
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <shared_mutex>

#include "awfm_matrix_kernel.h"

extern "C" {

enum AwFmReturnCode awfmGpuAlignChainsMatrix(AwFmGpuIndex *g, const struct AwFmVerifyInputs *dIn, const uint32_t *dSlots, uint64_t numReads,
                                             uint32_t maxCandidates, uint32_t bandPad, uint32_t maxDrift,
                                             const struct AwFmMatrixScoring *scoring, uint32_t maxOps, uint32_t maxRows,
                                             const struct AwFmAffineOutputs *dOut, void *dScratch, void *stream) {
  if (!g) {
    setError("awfmGpuAlignChainsMatrix: null image");
    return AwFmNullPtrError;
  }
  if (numReads == 0) return AwFmSuccess;
  const char *name = "awfmGpuAlignChainsMatrix";
  enum AwFmReturnCode rc = alignChainsArgumentsRefused(
      name, dIn, dSlots, scoring, [&] { return matrixScoringRefused(name, scoring); }, numReads, maxCandidates, bandPad, maxDrift, maxOps, maxRows,
      dOut, dScratch);
  if (rc != AwFmSuccess) return rc;
  DeviceGuard guard(g->device);
  AwFmGpuImage *image = g->image;
  std::shared_lock<std::shared_mutex> lock(image->recordMutex); /* neither text nor record table is replaced before the launch */
  if ((rc = textMissing(name, image)) != AwFmSuccess) return rc;
  DevAffineMatrixParams p{};
  unsigned group;
  dim3 grid;
  const dim3 block(kAffineThreads);
  alignChainsParams(g, dIn, dSlots, numReads, maxCandidates, bandPad, maxDrift, maxOps, maxRows, dOut, dScratch, p, group, grid);
  p.open = (int)(scoring->gapOpen + scoring->gapExtend);
  p.extend = (int)scoring->gapExtend;
  memcpy(p.matrix, scoring->substitution, sizeof p.matrix);
  AWFM_LAUNCH_BAND_KERNEL(alignChainsMatrixKernel, group, grid, block, stream, p);
  AWFM_HIP_TRY(hipGetLastError(), AwFmGeneralFailure);
  return AwFmSuccess;
}

}  // extern "C"
