/*
 * awfm_gpu_align.hip -- "chain alignment" on the device (include/awfm_gpu.h): awfmGpuAlignChains and the size of its trace
 * arena.  The kernel is awfm_align_kernel.h, the host twin and checker awfm_align.c.
 */
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <shared_mutex>

#include "awfm_align_kernel.h"

/* the waves of the persistent grid: the launch and the arena's size come from this one number */
static uint64_t alignGridWaves(const AwFmGpuIndex *g) { return (uint64_t)g->numCUs * kAlignBlocksPerCU * (kAlignThreads / 64u); }

extern "C" {

uint64_t awfmGpuAlignChainsScratchBytes(const AwFmGpuIndex *g, uint32_t maxRows) {
  if (!g || maxRows < 1 || maxRows > AWFM_ALIGN_MAX_LENGTH) return 0;
  return alignGridWaves(g) * kAlignRowBytes * maxRows;
}

enum AwFmReturnCode awfmGpuAlignChains(AwFmGpuIndex *g, const struct AwFmVerifyInputs *dIn, const uint32_t *dSlots, uint64_t numReads,
                                       uint32_t maxCandidates, uint32_t bandPad, uint32_t maxDrift, uint32_t maxOps, uint32_t maxRows,
                                       const struct AwFmAlignOutputs *dOut, void *dScratch, void *stream) {
  if (!g) {
    setError("awfmGpuAlignChains: null image");
    return AwFmNullPtrError;
  }
  if (numReads == 0) return AwFmSuccess;
  const char *name = "awfmGpuAlignChains";
  const uint64_t band = (uint64_t)maxDrift + 2ull * bandPad + 1ull;
  enum AwFmReturnCode rc = chainArgumentsRefused(name, dIn, dOut && dSlots && dScratch, numReads, maxCandidates, band);
  if (rc != AwFmSuccess) return rc;
  if (maxOps < 1 || maxOps > AWFM_ALIGN_MAX_OPS || maxRows < 1 || maxRows > AWFM_ALIGN_MAX_LENGTH) {
    setCallError(name, "maxOps is 1 to 4096 and maxRows 1 to 65536");
    return AwFmIllegalPositionError;
  }
  if ((uintptr_t)dScratch & 15u) {
    setCallError(name, "the scratch is aligned to 16 bytes");
    return AwFmIllegalPositionError;
  }
  DeviceGuard guard(g->device);
  AwFmGpuImage *image = g->image;
  std::shared_lock<std::shared_mutex> lock(image->recordMutex); /* neither text nor record table is replaced before the launch */
  if ((rc = textMissing(name, image)) != AwFmSuccess) return rc;
  DevAlignParams p{};
  p.in = *dIn;
  p.out = *dOut;
  p.chosen = dSlots;
  p.text = (const unsigned char *)image->dText;
  p.length = image->textLength;
  p.ends = image->records.ends;
  p.numRecords = image->records.numRecords;
  p.numReads = numReads;
  p.arena = (unsigned char *)dScratch;
  p.slots = maxCandidates;
  p.pad = bandPad;
  p.drift = maxDrift;
  p.amino = g->amino ? 1u : 0u;
  p.maxOps = maxOps;
  p.maxRows = maxRows;
  const unsigned group = bandGroup(band, "align_group");
  /* persistent grid over reads, a group each: never more waves than the arena has room for */
  const uint64_t perBlock = (uint64_t)(kAlignThreads / group), blocks = (numReads + perBlock - 1u) / perBlock;
  const uint64_t resident = alignGridWaves(g) / (kAlignThreads / 64u);
  const dim3 grid((unsigned)(blocks < resident ? blocks : resident)), block(kAlignThreads);
  AWFM_LAUNCH_BAND_KERNEL(alignChainsKernel, group, grid, block, stream, p);
  AWFM_HIP_TRY(hipGetLastError(), AwFmGeneralFailure);
  return AwFmSuccess;
}

}  // extern "C"
