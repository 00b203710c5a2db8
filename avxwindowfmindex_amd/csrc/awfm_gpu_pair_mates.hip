/*
 * awfm_gpu_pair_mates.hip -- "pair mates" on the device (include/awfm_gpu.h): awfmGpuPairMates and awfmGpuReverseComplementReads, and
 * awfmGpuPairMatesEstimated of "insert size", the same launch with the interval in device memory.
 * The kernels are awfm_pair_mates_kernel.h, the host twins and checkers awfm_pair_mates.c.  One launch each, no scratch, none of
 * the handle's scratch slots, nothing of the image but its device.
 */
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "awfm_pair_mates_kernel.h"

extern "C" {

/* awfmGpuPairMates (dEstimate NULL: the interval is params') and awfmGpuPairMatesEstimated (the interval lies in device memory and
 * the kernel validates it) */
static enum AwFmReturnCode pairMatesLaunch(const char *name, AwFmGpuIndex *g, const struct AwFmPairInputs *dIn, uint64_t numPairs,
                                           uint32_t maxCandidates, const struct AwFmPairParams *params, const struct AwFmInsertEstimate *dEstimate,
                                           bool estimated, const struct AwFmPairOutputs *dOut, void *stream) {
  char message[160];
  if (!g) {
    snprintf(message, sizeof message, "%s: null image", name);
    setError(message);
    return AwFmNullPtrError;
  }
  if (numPairs == 0) return AwFmSuccess;
  if (!dIn || !dOut || !params || (estimated && !dEstimate) || !dIn->readOffsets || !dIn->sequences || !dIn->slotScores || !dIn->slotReadEnds ||
      !dIn->slotTextEnds) {
    snprintf(message, sizeof message, "%s: null argument", name);
    setError(message);
    return AwFmNullPtrError;
  }
  if (numPairs >= (1ull << 31) || maxCandidates < 1 || maxCandidates > AWFM_CANDIDATES_MAX_SLOTS) {
    snprintf(message, sizeof message, "%s: read numbers are 32-bit, and a read has 1 to 16 slots", name);
    setError(message);
    return AwFmIllegalPositionError;
  }
  if ((!estimated && (params->minInsert > params->maxInsert || params->minInsert < -AWFM_PAIR_MAX_INSERT || params->maxInsert > AWFM_PAIR_MAX_INSERT)) ||
      params->mapqCap > AWFM_SCORE_MAX_MAPQ) {
    snprintf(message, sizeof message, "%s: minInsert <= maxInsert, both within 2^40 of 0, and mapqCap is 0 to 254", name);
    setError(message);
    return AwFmIllegalPositionError;
  }
  DeviceGuard guard(g->device);
  DevPairParams p{};
  p.in = *dIn;
  p.out = *dOut;
  p.numPairs = numPairs;
  p.minInsert = estimated ? 0 : params->minInsert;
  p.maxInsert = estimated ? 0 : params->maxInsert;
  p.pad = (long long)params->windowPad;
  p.slots = maxCandidates;
  p.floor = params->minScore > 1u ? params->minScore : 1u;
  p.penalty = params->unpairedPenalty;
  p.cap = params->mapqCap;
  p.estimate = estimated ? dEstimate : nullptr;
  unsigned group = maxCandidates <= 4u ? 16u : 64u;
  if (const char *env = awfmGpuDiag("pair_group")) { /* tests: a wave per pair where sixteen lanes would do */
    if ((unsigned)atoi(env) == 64u) group = 64u;
  }
  /* persistent grid over pairs, a group each */
  const uint64_t perBlock = kPairThreads / group, blocks = (numPairs + perBlock - 1u) / perBlock;
  const uint64_t resident = (uint64_t)g->numCUs * kPairBlocksPerCU;
  const dim3 grid((unsigned)(blocks < resident ? blocks : resident)), block(kPairThreads);
  hipStream_t s = (hipStream_t)stream;
  if (group == 16u) hipLaunchKernelGGL(pairMatesKernel<16>, grid, block, 0, s, p);
  else hipLaunchKernelGGL(pairMatesKernel<64>, grid, block, 0, s, p);
  AWFM_HIP_TRY(hipGetLastError(), AwFmGeneralFailure);
  return AwFmSuccess;
}

enum AwFmReturnCode awfmGpuPairMates(AwFmGpuIndex *g, const struct AwFmPairInputs *dIn, uint64_t numPairs, uint32_t maxCandidates,
                                     const struct AwFmPairParams *params, const struct AwFmPairOutputs *dOut, void *stream) {
  return pairMatesLaunch("awfmGpuPairMates", g, dIn, numPairs, maxCandidates, params, nullptr, false, dOut, stream);
}

enum AwFmReturnCode awfmGpuPairMatesEstimated(AwFmGpuIndex *g, const struct AwFmPairInputs *dIn, uint64_t numPairs, uint32_t maxCandidates,
                                              const struct AwFmPairParams *params, const struct AwFmInsertEstimate *dEstimate,
                                              const struct AwFmPairOutputs *dOut, void *stream) {
  return pairMatesLaunch("awfmGpuPairMatesEstimated", g, dIn, numPairs, maxCandidates, params, dEstimate, true, dOut, stream);
}

enum AwFmReturnCode awfmGpuReverseComplementReads(AwFmGpuIndex *g, const uint8_t *dReadChars, uint64_t numReadChars,
                                                  const uint64_t *dReadOffsets, uint64_t numReads, uint32_t which, uint8_t *dOut,
                                                  uint64_t *dNumMalformed, void *stream) {
  if (!g) {
    setError("awfmGpuReverseComplementReads: null image");
    return AwFmNullPtrError;
  }
  if (numReads == 0) return AwFmSuccess;
  if (!dReadOffsets || (!dReadChars && numReadChars != 0)) {
    setError("awfmGpuReverseComplementReads: null argument");
    return AwFmNullPtrError;
  }
  if (which > AWFM_COMPLEMENT_EVEN) {
    setError("awfmGpuReverseComplementReads: which is AWFM_COMPLEMENT_ALL, _ODD or _EVEN");
    return AwFmIllegalPositionError;
  }
  if (dOut && numReadChars && (uintptr_t)dReadChars < (uintptr_t)dOut + numReadChars && (uintptr_t)dOut < (uintptr_t)dReadChars + numReadChars) {
    setError("awfmGpuReverseComplementReads: input and output overlap");
    return AwFmIllegalPositionError;
  }
  DeviceGuard guard(g->device);
  DevComplementParams p{};
  p.chars = dReadChars;
  p.out = dOut;
  p.offsets = (const unsigned long long *)dReadOffsets;
  p.numChars = numReadChars;
  p.numReads = numReads;
  p.numMalformed = (unsigned long long *)dNumMalformed;
  p.which = which;
  /* persistent grid over reads, a wave each */
  const uint64_t perBlock = kComplementThreads / 64u, blocks = (numReads + perBlock - 1u) / perBlock;
  const uint64_t resident = (uint64_t)g->numCUs * kComplementBlocksPerCU;
  const dim3 grid((unsigned)(blocks < resident ? blocks : resident)), block(kComplementThreads);
  hipLaunchKernelGGL(reverseComplementKernel, grid, block, 0, (hipStream_t)stream, p);
  AWFM_HIP_TRY(hipGetLastError(), AwFmGeneralFailure);
  return AwFmSuccess;
}

}  // extern "C"
