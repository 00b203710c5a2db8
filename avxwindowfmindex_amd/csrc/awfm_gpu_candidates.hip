/*
 * awfm_gpu_candidates.hip -- awfmGpuReadCandidates and awfmGpuReadCandidatesScratchBytes (include/awfm_gpu.h, "candidate
 * loci"): the located seeds of every read grouped into candidate loci on the device.  The kernels are awfm_candidates_kernel.h,
 * the host twin and checker is awfm_candidates.c; the refusals, the scratch and the launch of the two tiers are
 * awfm_hits_kernel.h's.  The reference has no analogue (it stops at positions: ref src/AwFmParallelSearch.c:315-365).
 */
#include <hip/hip_runtime.h>

#include "awfm_candidates_kernel.h"

extern "C" {

uint64_t awfmGpuReadCandidatesScratchBytes(uint64_t numReads) { return hitsScratchBytes(numReads); }

enum AwFmReturnCode awfmGpuReadCandidates(AwFmGpuIndex *g, const struct AwFmCandidateInputs *dIn, uint64_t numReads,
                                          uint32_t maxHitsPerSeed, uint32_t band, uint32_t minVotes, uint32_t maxCandidates,
                                          const struct AwFmCandidateOutputs *dOut, void *dScratch, void *stream) {
  if (!g) {
    setError("awfmGpuReadCandidates: null image");
    return AwFmNullPtrError;
  }
  if (numReads == 0) return AwFmSuccess;
  const enum AwFmReturnCode refused = hitsArgumentsRefused("awfmGpuReadCandidates", dIn, dOut && dScratch, numReads, maxCandidates);
  if (refused != AwFmSuccess) return refused;
  DevCandidateParams p{};
  p.in = *dIn;
  p.out = *dOut;
  p.numReads = numReads;
  p.maxHitsPerSeed = maxHitsPerSeed;
  p.band = band;
  p.minVotes = minVotes ? minVotes : 1u;
  p.slots = maxCandidates;
  return launchTiers(g, p, "candidates_tier", kCandidatesWaveLimit, readCandidatesWaveKernel, kCandidatesWaveThreads,
                     readCandidatesGroupKernel, kCandidatesGroupThreads, 0u, dScratch, stream);
}

}  // extern "C"
