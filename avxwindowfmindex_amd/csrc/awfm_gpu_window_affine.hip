/*
 * awfm_gpu_window_affine.hip -- "window scores" on the device (include/awfm_gpu.h): awfmGpuScoreWindowsAffine and the size of its
 * scratch.  The kernel is awfm_window_affine_kernel.h, the host twin and checker awfm_window_affine.c.  One launch, none of the
 * handle's scratch slots.
 */
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <shared_mutex>

#include "awfm_window_affine_kernel.h"

/* the waves of a full grid: the arena has a share for each */
static uint64_t windowGridWaves(const AwFmGpuIndex *g) { return (uint64_t)g->numCUs * kWinAffBlocksPerCU * (kWinAffThreads / 64u); }

extern "C" {

uint64_t awfmGpuScoreWindowsAffineScratchBytes(const AwFmGpuIndex *g, uint32_t maxLength) {
  if (!g || maxLength < 1 || maxLength > AWFM_WINDOW_MAX_LENGTH) return 0;
  return windowGridWaves(g) * 2ull * kWinAffEntryBytes * maxLength;
}

enum AwFmReturnCode awfmGpuScoreWindowsAffine(AwFmGpuIndex *g, const struct AwFmWindowInputs *dIn, uint64_t numReads,
                                              const struct AwFmAlignScoring *scoring, uint32_t minScore, uint32_t slotStride,
                                              uint32_t slotColumn, uint32_t maxLength, const struct AwFmWindowOutputs *dOut, void *dScratch,
                                              void *stream) {
  if (!g) {
    setError("awfmGpuScoreWindowsAffine: null image");
    return AwFmNullPtrError;
  }
  if (numReads == 0) return AwFmSuccess;
  if (!dIn || !dOut || !scoring || !dScratch || !dIn->readOffsets || !dIn->windowSequences || !dIn->windowBegins || !dIn->windowEnds ||
      (!dIn->readChars && dIn->numReadChars != 0)) {
    setError("awfmGpuScoreWindowsAffine: null argument");
    return AwFmNullPtrError;
  }
  if (numReads >= (1ull << 32) || slotStride < 1 || slotStride > AWFM_CANDIDATES_MAX_SLOTS || slotColumn >= slotStride) {
    setError("awfmGpuScoreWindowsAffine: read numbers are 32-bit, slotStride is 1 to 16 and slotColumn lies below it");
    return AwFmIllegalPositionError;
  }
  if (maxLength < 1 || maxLength > AWFM_WINDOW_MAX_LENGTH || ((uintptr_t)dScratch & 15u)) {
    setError("awfmGpuScoreWindowsAffine: maxLength is 1 to 4096, and the scratch is aligned to 16 bytes");
    return AwFmIllegalPositionError;
  }
  if (scoringRefused("awfmGpuScoreWindowsAffine", scoring) != AwFmSuccess) return AwFmIllegalPositionError;
  DeviceGuard guard(g->device);
  AwFmGpuImage *image = g->image;
  std::shared_lock<std::shared_mutex> lock(image->recordMutex); /* neither text nor record table is replaced before the launch */
  if (!image->dText) {
    setError("awfmGpuScoreWindowsAffine: the image has no text (awfmGpuIndexSetText uploads it)");
    return AwFmUnsupportedVersionError;
  }
  DevWindowParams p{};
  p.in = *dIn;
  p.out = *dOut;
  p.text = (const unsigned char *)image->dText;
  p.length = image->textLength;
  p.ends = image->records.ends;
  p.numRecords = image->records.numRecords;
  p.numReads = numReads;
  p.arena = (uint4 *)dScratch;
  p.maxLength = maxLength;
  p.stride = slotStride;
  p.column = slotColumn;
  p.amino = g->amino ? 1u : 0u;
  p.floor = minScore > 1u ? minScore : 1u;
  p.match = (int)scoring->match;
  p.mismatch = (int)scoring->mismatch;
  p.open = (int)(scoring->gapOpen + scoring->gapExtend);
  p.extend = (int)scoring->gapExtend;
  if (const char *env = awfmGpuDiag("window_q")) { /* tests: one Q for every read, so that narrow windows go in column blocks */
    const unsigned forced = (unsigned)atoi(env);
    if (forced == 4u || forced == 8u || forced == 12u) p.forcedQ = forced;
  }
  /* persistent grid over reads, a wave each */
  const uint64_t perBlock = kWinAffThreads / 64u, blocks = (numReads + perBlock - 1u) / perBlock;
  const uint64_t resident = (uint64_t)g->numCUs * kWinAffBlocksPerCU;
  const dim3 grid((unsigned)(blocks < resident ? blocks : resident)), block(kWinAffThreads);
  hipLaunchKernelGGL(scoreWindowsAffineKernel, grid, block, 0, (hipStream_t)stream, p);
  AWFM_HIP_TRY(hipGetLastError(), AwFmGeneralFailure);
  return AwFmSuccess;
}

}  // extern "C"
