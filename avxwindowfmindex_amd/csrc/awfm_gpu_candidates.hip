/*
 * awfm_gpu_candidates.hip -- awfmGpuReadCandidates and awfmGpuReadCandidatesScratchBytes (include/awfm_gpu.h, "candidate
 * loci"): the located seeds of every read grouped into candidate loci on the device.  The kernels are awfm_candidates_kernel.h,
 * the host twin and checker is awfm_candidates.c.  The reference has no analogue (it stops at positions:
 * ref src/AwFmParallelSearch.c:315-365).
 */
#include <hip/hip_runtime.h>
#include <cstring>

#include "awfm_candidates_kernel.h"

namespace {
constexpr uint64_t kCounterBytes = 16; /* the worklist's length, ahead of the worklist */
}

extern "C" {

uint64_t awfmGpuReadCandidatesScratchBytes(uint64_t numReads) { return kCounterBytes + alignUp(numReads * 4u, 16); }

enum AwFmReturnCode awfmGpuReadCandidates(AwFmGpuIndex *g, const struct AwFmCandidateInputs *dIn, uint64_t numReads,
                                          uint32_t maxHitsPerSeed, uint32_t band, uint32_t minVotes, uint32_t maxCandidates,
                                          const struct AwFmCandidateOutputs *dOut, void *dScratch, void *stream) {
  if (!g) {
    setError("awfmGpuReadCandidates: null image");
    return AwFmNullPtrError;
  }
  if (numReads == 0) return AwFmSuccess;
  if (!dIn || !dOut || !dScratch || !dIn->readSeedOffsets || !dIn->seedEnds || !dIn->hitOffsets || !dIn->positions) {
    setError("awfmGpuReadCandidates: null argument");
    return AwFmNullPtrError;
  }
  if (!dIn->seedLengths && dIn->fixedLength == 0) {
    setError("awfmGpuReadCandidates: the seeds need their lengths or a fixed length");
    return AwFmNullPtrError;
  }
  if (numReads >= (1ull << 32) || maxCandidates < 1 || maxCandidates > AWFM_CANDIDATES_MAX_SLOTS) {
    setError("awfmGpuReadCandidates: read numbers are 32-bit, and a read has 1 to 16 slots");
    return AwFmIllegalPositionError;
  }
  DeviceGuard guard(g->device);
  DevCandidateParams p{};
  p.in = *dIn;
  p.out = *dOut;
  p.numReads = numReads;
  p.maxHitsPerSeed = maxHitsPerSeed;
  p.band = band;
  p.minVotes = minVotes ? minVotes : 1u;
  p.slots = maxCandidates;
  p.waveLimit = kCandidatesWaveLimit;
  /* tests: `group` sends every read with a kept hit through the workgroup tier; `wave` names the default, in which every
   * read that fits the wave tier already takes it */
  if (const char *env = awfmGpuDiag("candidates_tier")) {
    if (!strcmp(env, "group")) p.waveLimit = 0;
  }
  p.counter = (unsigned long long *)dScratch;
  p.worklist = (unsigned *)((uint8_t *)dScratch + kCounterBytes);
  hipStream_t s = (hipStream_t)stream;
  AWFM_HIP_TRY(hipMemsetAsync(dScratch, 0, kCounterBytes, s), AwFmGeneralFailure);
  /* persistent grids: 16 waves per CU of the wave tier, the two workgroups per CU that the workgroup tier's LDS leaves */
  const uint64_t waveBlocks = (uint64_t)g->numCUs * 16u, groupBlocks = (uint64_t)g->numCUs * 2u;
  hipLaunchKernelGGL(readCandidatesWaveKernel, dim3((unsigned)(numReads < waveBlocks ? numReads : waveBlocks)), dim3(kCandidatesWaveThreads), 0,
                     s, p);
  AWFM_HIP_TRY(hipGetLastError(), AwFmGeneralFailure);
  hipLaunchKernelGGL(readCandidatesGroupKernel, dim3((unsigned)(numReads < groupBlocks ? numReads : groupBlocks)),
                     dim3(kCandidatesGroupThreads), 0, s, p);
  AWFM_HIP_TRY(hipGetLastError(), AwFmGeneralFailure);
  return AwFmSuccess;
}

}  // extern "C"
