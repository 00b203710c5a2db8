/*
 * awfm_gpu_insert.hip -- "insert size" on the device (include/awfm_gpu.h): awfmGpuInsertHistogram and awfmGpuInsertInterval.
 * The kernels are awfm_insert_kernel.h, the host twins and checkers awfm_insert.c.  One launch each, no scratch, none of the
 * handle's scratch slots, nothing of the image but its device.  (awfmGpuPairMatesEstimated lives with awfmGpuPairMates.)
 */
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>

#include "awfm_insert_kernel.h"

namespace {

/* what all four calls of the section ask of their params (awfm_insert.c has the same) */
bool insertParamsAreLegal(const struct AwFmInsertParams *q) {
  if (q->lowTemplate > q->highTemplate || q->lowTemplate < -AWFM_PAIR_MAX_INSERT || q->highTemplate > AWFM_PAIR_MAX_INSERT) return false;
  if ((uint64_t)(q->highTemplate - q->lowTemplate) >= AWFM_INSERT_MAX_BINS) return false;
  if (q->spread > AWFM_INSERT_MAX_SPREAD) return false;
  return q->fallbackMin <= q->fallbackMax && q->fallbackMin >= -AWFM_PAIR_MAX_INSERT && q->fallbackMax <= AWFM_PAIR_MAX_INSERT;
}

#define AWFM_INSERT_PARAMS_RULE ": lowTemplate <= highTemplate with at most 65536 bins, spread 0 to 16, fallbackMin <= fallbackMax, all within 2^40 of 0"

}  // namespace

extern "C" {

enum AwFmReturnCode awfmGpuInsertHistogram(AwFmGpuIndex *g, const struct AwFmPairInputs *dIn, uint64_t numPairs, uint32_t maxCandidates,
                                           const struct AwFmInsertParams *params, uint64_t *dHistogram, uint64_t *dNumSamples,
                                           uint64_t *dNumOutside, void *stream) {
  if (!g) {
    setError("awfmGpuInsertHistogram: null image");
    return AwFmNullPtrError;
  }
  if (numPairs == 0) return AwFmSuccess;
  if (!dIn || !params || !dHistogram || !dIn->readOffsets || !dIn->sequences || !dIn->slotScores || !dIn->slotReadEnds || !dIn->slotTextEnds) {
    setError("awfmGpuInsertHistogram: null argument");
    return AwFmNullPtrError;
  }
  if (numPairs >= (1ull << 31) || maxCandidates < 1 || maxCandidates > AWFM_CANDIDATES_MAX_SLOTS) {
    setError("awfmGpuInsertHistogram: read numbers are 32-bit, and a read has 1 to 16 slots");
    return AwFmIllegalPositionError;
  }
  if (!insertParamsAreLegal(params)) {
    setError("awfmGpuInsertHistogram" AWFM_INSERT_PARAMS_RULE);
    return AwFmIllegalPositionError;
  }
  DeviceGuard guard(g->device);
  DevInsertParams p{};
  p.in = *dIn;
  p.histogram = (unsigned long long *)dHistogram;
  p.numSamples = (unsigned long long *)dNumSamples;
  p.numOutside = (unsigned long long *)dNumOutside;
  p.numPairs = numPairs;
  p.low = params->lowTemplate;
  p.high = params->highTemplate;
  p.slots = maxCandidates;
  p.floor = params->minScore > 1u ? params->minScore : 1u;
  p.minQuality = params->minQuality;
  p.bins = (unsigned)(params->highTemplate - params->lowTemplate) + 1u;
  bool lds = p.bins <= kInsertLdsBins;
  if (const char *env = awfmGpuDiag("insert_tier")) { /* tests: global atomics where a private histogram would fit */
    if (!strcmp(env, "global")) lds = false;
  }
  /* persistent grid over pairs, a thread each; a workgroup gets at least kInsertPairsPerBlock of them */
  const uint64_t blocks = (numPairs + kInsertPairsPerBlock - 1u) / kInsertPairsPerBlock;
  const uint64_t resident = (uint64_t)g->numCUs * kInsertBlocksPerCU;
  const dim3 grid((unsigned)(blocks < resident ? blocks : resident)), block(kInsertThreads);
  hipStream_t s = (hipStream_t)stream;
  if (lds) hipLaunchKernelGGL(insertHistogramKernel<true>, grid, block, 0, s, p);
  else hipLaunchKernelGGL(insertHistogramKernel<false>, grid, block, 0, s, p);
  AWFM_HIP_TRY(hipGetLastError(), AwFmGeneralFailure);
  return AwFmSuccess;
}

enum AwFmReturnCode awfmGpuInsertInterval(AwFmGpuIndex *g, const uint64_t *dHistogram, const struct AwFmInsertParams *params,
                                          struct AwFmInsertEstimate *dEstimate, void *stream) {
  if (!g) {
    setError("awfmGpuInsertInterval: null image");
    return AwFmNullPtrError;
  }
  if (!dHistogram || !params || !dEstimate) {
    setError("awfmGpuInsertInterval: null argument");
    return AwFmNullPtrError;
  }
  if (!insertParamsAreLegal(params)) {
    setError("awfmGpuInsertInterval" AWFM_INSERT_PARAMS_RULE);
    return AwFmIllegalPositionError;
  }
  DeviceGuard guard(g->device);
  DevIntervalParams p{};
  p.histogram = (const unsigned long long *)dHistogram;
  p.estimate = dEstimate;
  p.low = params->lowTemplate;
  p.fallbackMin = params->fallbackMin;
  p.fallbackMax = params->fallbackMax;
  p.bins = (unsigned)(params->highTemplate - params->lowTemplate) + 1u;
  p.spread = params->spread;
  p.minSamples = params->minSamples;
  hipLaunchKernelGGL(insertIntervalKernel, dim3(1), dim3(kIntervalThreads), 0, (hipStream_t)stream, p);
  AWFM_HIP_TRY(hipGetLastError(), AwFmGeneralFailure);
  return AwFmSuccess;
}

}  // extern "C"
