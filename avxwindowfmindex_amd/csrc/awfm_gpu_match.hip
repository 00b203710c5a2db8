/*
 * awfm_gpu_match.hip -- awfmGpuLongestSuffixMatches (include/awfm_gpu.h): the launch of longestMatchKernel
 * (awfm_match_kernel.h).  One kernel, asynchronous on the caller's stream; like the general search kernel it needs no scratch
 * memory, so it takes none of the handle's slots and two streams may run it on one image at the same time.
 * ref src/AwFmSearch.c:27-159 (the steps), src/AwFmIndex.h:477-512 (what they are published for).
 */
#include <hip/hip_runtime.h>

#include "awfm_match_kernel.h"

namespace {

template <bool AMINO, bool NARROW, bool PAIR>
void launchMatch(const AwFmGpuIndex *g, hipStream_t s, const uint8_t *dChars, const unsigned long long *starts,
                 const unsigned long long *ends, uint32_t fixedLength, unsigned long long nq, uint32_t minLength, unsigned *lengths,
                 ulonglong2 *rng, unsigned *counts) {
  /* PAIR: the 16 pair bases of every superblock in dynamic LDS where they fit, as the general kernel has them */
  const bool inLds = PAIR && NARROW && awfmPairSuperInLds(g);
  const size_t lds = inLds ? (size_t)g->image->dev.numPairSuper * 64u : 0u;
  DevIndex view = g->image->dev;
  view.pairSuperInLds = inLds ? 1u : 0u;
  const unsigned grid = gridFor(nq, g, longestMatchKernel<AMINO, NARROW, PAIR>, kThreads / kMatchLanes, lds);
  hipLaunchKernelGGL((longestMatchKernel<AMINO, NARROW, PAIR>), dim3(grid), dim3(kThreads), lds, s, view, dChars, starts, ends,
                     fixedLength, nq, minLength, lengths, rng, counts);
}

}  // namespace

extern "C" enum AwFmReturnCode awfmGpuLongestSuffixMatches(AwFmGpuIndex *g, const uint8_t *dChars, const uint64_t *dStarts,
                                                           const uint64_t *dEnds, uint32_t fixedLength, uint64_t numQueries,
                                                           uint32_t minLength, uint32_t *dMatchLengths,
                                                           struct AwFmSearchRange *dRanges, uint32_t *dCounts, void *stream) {
  if (!g) {
    setError("awfmGpuLongestSuffixMatches: null image");
    return AwFmNullPtrError;
  }
  if (numQueries == 0) return AwFmSuccess;
  if (!dChars || (dStarts == nullptr) != (dEnds == nullptr) || (!dStarts && fixedLength == 0)) {
    setError("awfmGpuLongestSuffixMatches: queries need dChars and either dStarts and dEnds or fixedLength");
    return AwFmNullPtrError;
  }
  DeviceGuard guard(g->device);
  hipStream_t s = (hipStream_t)stream;
  const bool narrow = awfmImageNarrow(g);
  const unsigned long long *starts = (const unsigned long long *)dStarts, *ends = (const unsigned long long *)dEnds;
#define AWFM_MATCH_GO(AM, NR, PR) \
  launchMatch<AM, NR, PR>(g, s, dChars, starts, ends, fixedLength, numQueries, minLength, dMatchLengths, (ulonglong2 *)dRanges, dCounts)
  if (g->amino) {
    if (narrow) AWFM_MATCH_GO(true, true, false);
    else AWFM_MATCH_GO(true, false, false);
  } else if (g->image->dev.pairBlocks) {
    if (narrow) AWFM_MATCH_GO(false, true, true);
    else AWFM_MATCH_GO(false, false, true);
  } else {
    if (narrow) AWFM_MATCH_GO(false, true, false);
    else AWFM_MATCH_GO(false, false, false);
  }
#undef AWFM_MATCH_GO
  AWFM_HIP_TRY(hipGetLastError(), AwFmGeneralFailure);
  return AwFmSuccess;
}
