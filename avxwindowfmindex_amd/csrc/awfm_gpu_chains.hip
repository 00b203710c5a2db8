/*
 * awfm_gpu_chains.hip -- awfmGpuReadChains and awfmGpuReadChainsScratchBytes (include/awfm_gpu.h, "read chains"): the best
 * colinear chain of every candidate slot of every read on the device.  The kernels are awfm_chains_kernel.h, the host twin and
 * checker is awfm_chains.c.  The reference has no analogue (it stops at positions: ref src/AwFmParallelSearch.c:315-365).
 */
#include <hip/hip_runtime.h>
#include <cstring>

#include "awfm_chains_kernel.h"

namespace {
constexpr uint64_t kCounterBytes = 16; /* the worklist's length, ahead of the worklist */
}

extern "C" {

uint64_t awfmGpuReadChainsScratchBytes(uint64_t numReads) { return kCounterBytes + alignUp(numReads * 4u, 16); }

enum AwFmReturnCode awfmGpuReadChains(AwFmGpuIndex *g, const struct AwFmCandidateInputs *dIn, uint64_t numReads, uint32_t maxHitsPerSeed,
                                      uint32_t band, uint32_t maxCandidates, const uint32_t *dSequences, const int64_t *dDiagonals,
                                      const uint32_t *dDiagonalSpans, uint32_t lookback, uint32_t gapPenalty,
                                      const struct AwFmChainOutputs *dOut, void *dScratch, void *stream) {
  if (!g) {
    setError("awfmGpuReadChains: null image");
    return AwFmNullPtrError;
  }
  if (numReads == 0) return AwFmSuccess;
  if (!dIn || !dOut || !dScratch || !dIn->readSeedOffsets || !dIn->seedEnds || !dIn->hitOffsets || !dIn->positions || !dSequences ||
      !dDiagonals || !dDiagonalSpans) {
    setError("awfmGpuReadChains: null argument");
    return AwFmNullPtrError;
  }
  if (!dIn->seedLengths && dIn->fixedLength == 0) {
    setError("awfmGpuReadChains: the seeds need their lengths or a fixed length");
    return AwFmNullPtrError;
  }
  if (numReads >= (1ull << 32) || maxCandidates < 1 || maxCandidates > AWFM_CANDIDATES_MAX_SLOTS) {
    setError("awfmGpuReadChains: read numbers are 32-bit, and a read has 1 to 16 slots");
    return AwFmIllegalPositionError;
  }
  if (lookback < 1 || lookback > AWFM_CHAINS_MAX_LOOKBACK) {
    setError("awfmGpuReadChains: an anchor looks back at 1 to 64 anchors");
    return AwFmIllegalPositionError;
  }
  DeviceGuard guard(g->device);
  DevChainParams p{};
  p.in = *dIn;
  p.out = *dOut;
  p.sequences = dSequences;
  p.diagonals = (const long long *)dDiagonals;
  p.spans = dDiagonalSpans;
  p.numReads = numReads;
  p.maxHitsPerSeed = maxHitsPerSeed;
  p.band = band;
  p.slots = maxCandidates;
  p.lookback = lookback;
  p.gapPenalty = gapPenalty;
  p.waveLimit = kChainsWaveLimit;
  /* tests: `group` sends every read with an anchor through the workgroup tier; `wave` names the default, in which every read
   * that fits the wave tier already takes it */
  if (const char *env = awfmGpuDiag("chains_tier")) {
    if (!strcmp(env, "group")) p.waveLimit = 0;
  }
  p.counter = (unsigned long long *)dScratch;
  p.worklist = (unsigned *)((uint8_t *)dScratch + kCounterBytes);
  hipStream_t s = (hipStream_t)stream;
  /* the workgroup tier's LDS is beyond what a kernel gets without asking.  The limit belongs to the kernel ON A DEVICE: it is
   * set under the guard at every call (a host-side table write), not once per process, which would leave every device but the
   * first call's without it */
  AWFM_HIP_TRY(hipFuncSetAttribute((const void *)readChainsGroupKernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kChainsGroupLdsBytes),
               AwFmGeneralFailure);
  AWFM_HIP_TRY(hipMemsetAsync(dScratch, 0, kCounterBytes, s), AwFmGeneralFailure);
  /* persistent grids: 16 waves per CU of the wave tier, the two workgroups per CU that the workgroup tier's LDS leaves */
  const uint64_t waveBlocks = (uint64_t)g->numCUs * 16u, groupBlocks = (uint64_t)g->numCUs * 2u;
  hipLaunchKernelGGL(readChainsWaveKernel, dim3((unsigned)(numReads < waveBlocks ? numReads : waveBlocks)), dim3(kChainsWaveThreads), 0, s, p);
  AWFM_HIP_TRY(hipGetLastError(), AwFmGeneralFailure);
  hipLaunchKernelGGL(readChainsGroupKernel, dim3((unsigned)(numReads < groupBlocks ? numReads : groupBlocks)), dim3(kChainsGroupThreads),
                     kChainsGroupLdsBytes, s, p);
  AWFM_HIP_TRY(hipGetLastError(), AwFmGeneralFailure);
  return AwFmSuccess;
}

}  // extern "C"
