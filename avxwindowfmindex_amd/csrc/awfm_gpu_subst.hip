/*
 * awfm_gpu_subst.hip -- awfmGpuOneSubstitutionSearch (include/awfm_gpu.h): the launches of oneSubstitutionFillKernel and
 * oneSubstitutionKernel (awfm_subst_kernel.h).  Two kernels, asynchronous on the caller's stream; no scratch memory, so the
 * call takes none of the handle's slots and two streams may run it on one image at the same time (as awfm_gpu_match.hip).
 * ref src/AwFmSearch.c:27-159, :317-358.
 */
#include <hip/hip_runtime.h>

#include "awfm_subst_kernel.h"

namespace {

template <bool AMINO, bool NARROW, bool TABLES>
void launchSubst(const AwFmGpuIndex *g, hipStream_t s, const uint8_t *dChars, const unsigned long long *offsets, uint32_t fixedLength,
                 unsigned long long nq, unsigned includeExact, const SubstOut &out) {
  const unsigned grid = gridFor(nq, g, oneSubstitutionKernel<AMINO, NARROW, TABLES>, kThreads / kSubstLanes);
  hipLaunchKernelGGL((oneSubstitutionKernel<AMINO, NARROW, TABLES>), dim3(grid), dim3(kThreads), 0, s, g->image->dev, dChars, offsets,
                     fixedLength, nq, includeExact, out);
}

}  // namespace

extern "C" enum AwFmReturnCode awfmGpuOneSubstitutionSearch(AwFmGpuIndex *g, const uint8_t *dChars, const uint64_t *dOffsets,
                                                            uint32_t fixedLength, uint64_t numQueries, int includeExact,
                                                            uint32_t *dHitQueries, uint32_t *dHitEdits,
                                                            struct AwFmSearchRange *dHitRanges, uint64_t capacity, uint64_t *dNumHits,
                                                            uint32_t *dVariantsPerQuery, uint64_t *dOccurrencesPerQuery, void *stream) {
  if (!g) {
    setError("awfmGpuOneSubstitutionSearch: null image");
    return AwFmNullPtrError;
  }
  if (numQueries == 0) return AwFmSuccess;
  if (numQueries >= (1ull << 32)) {
    setError("awfmGpuOneSubstitutionSearch: query numbers are 32-bit");
    return AwFmIllegalPositionError;
  }
  if (!dChars || (!dOffsets && fixedLength == 0)) {
    setError("awfmGpuOneSubstitutionSearch: queries need dChars and either dOffsets or fixedLength");
    return AwFmNullPtrError;
  }
  const bool lists = capacity != 0 && (dHitQueries || dHitEdits || dHitRanges);
  if (lists && !dNumHits) {
    setError("awfmGpuOneSubstitutionSearch: the lists are appended through dNumHits");
    return AwFmNullPtrError;
  }
  DeviceGuard guard(g->device);
  hipStream_t s = (hipStream_t)stream;
  SubstOut out;
  out.queries = lists ? dHitQueries : nullptr;
  out.edits = lists ? dHitEdits : nullptr;
  out.ranges = lists ? (ulonglong2 *)dHitRanges : nullptr;
  out.capacity = lists ? capacity : 0ull;
  out.count = (unsigned long long *)dNumHits;
  out.variants = dVariantsPerQuery;
  out.occurrences = (unsigned long long *)dOccurrencesPerQuery;
  if (out.count) {
    const unsigned long long blocks = (out.capacity + 255ull) / 256ull;
    const unsigned long long most = (unsigned long long)g->numCUs * 8ull;
    const unsigned grid = (unsigned)(blocks < most ? (blocks ? blocks : 1ull) : most);
    hipLaunchKernelGGL(oneSubstitutionFillKernel, dim3(grid), dim3(256), 0, s, out);
  }
  const bool narrow = awfmImageNarrow(g);
  /* the plain path: letter by letter, no table (awfmGpuIndexSetKernel with anything but AUTO or GROUP4) */
  const bool tables = !g->amino && (g->kernel == AWFM_GPU_KERNEL_AUTO || g->kernel == AWFM_GPU_KERNEL_GROUP4);
  const unsigned long long *offsets = (const unsigned long long *)dOffsets;
#define AWFM_SUBST_GO(AM, NR, TB) launchSubst<AM, NR, TB>(g, s, dChars, offsets, fixedLength, numQueries, includeExact ? 1u : 0u, out)
  if (g->amino) {
    if (narrow) AWFM_SUBST_GO(true, true, false);
    else AWFM_SUBST_GO(true, false, false);
  } else if (tables) {
    if (narrow) AWFM_SUBST_GO(false, true, true);
    else AWFM_SUBST_GO(false, false, true);
  } else {
    if (narrow) AWFM_SUBST_GO(false, true, false);
    else AWFM_SUBST_GO(false, false, false);
  }
#undef AWFM_SUBST_GO
  AWFM_HIP_TRY(hipGetLastError(), AwFmGeneralFailure);
  return AwFmSuccess;
}
