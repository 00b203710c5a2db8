/*
 * awfm_gpu_chains.hip -- awfmGpuReadChains and awfmGpuReadChainsScratchBytes (include/awfm_gpu.h, "read chains"): the best
 * colinear chain of every candidate slot of every read on the device.  The kernels are awfm_chains_kernel.h, the host twin and
 * checker is awfm_chains.c; the refusals it shares with the candidate call, the scratch and the launch of the two tiers are
 * awfm_hits_kernel.h's.  The reference has no analogue (it stops at positions: ref src/AwFmParallelSearch.c:315-365).
 */
#include <hip/hip_runtime.h>

#include "awfm_chains_kernel.h"

extern "C" {

uint64_t awfmGpuReadChainsScratchBytes(uint64_t numReads) { return hitsScratchBytes(numReads); }

enum AwFmReturnCode awfmGpuReadChains(AwFmGpuIndex *g, const struct AwFmCandidateInputs *dIn, uint64_t numReads, uint32_t maxHitsPerSeed,
                                      uint32_t band, uint32_t maxCandidates, const uint32_t *dSequences, const int64_t *dDiagonals,
                                      const uint32_t *dDiagonalSpans, uint32_t lookback, uint32_t gapPenalty,
                                      const struct AwFmChainOutputs *dOut, void *dScratch, void *stream) {
  if (!g) {
    setError("awfmGpuReadChains: null image");
    return AwFmNullPtrError;
  }
  if (numReads == 0) return AwFmSuccess;
  const enum AwFmReturnCode refused = hitsArgumentsRefused("awfmGpuReadChains", dIn, dOut && dScratch && dSequences && dDiagonals && dDiagonalSpans,
                                                           numReads, maxCandidates);
  if (refused != AwFmSuccess) return refused;
  if (lookback < 1 || lookback > AWFM_CHAINS_MAX_LOOKBACK) {
    setError("awfmGpuReadChains: an anchor looks back at 1 to 64 anchors");
    return AwFmIllegalPositionError;
  }
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
  return launchTiers(g, p, "chains_tier", kChainsWaveLimit, readChainsWaveKernel, kChainsWaveThreads, readChainsGroupKernel,
                     kChainsGroupThreads, kChainsGroupLdsBytes, dScratch, stream);
}

}  // extern "C"
