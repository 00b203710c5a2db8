/*
 * awfm_gpu_score_affine.hip -- "slot scores and mapping quality" on the device (include/awfm_gpu.h): awfmGpuScoreChainsAffine.  The
 * kernel is awfm_score_affine_kernel.h, the host twin and checker awfm_score_affine.c.  One launch, no scratch, none of the
 * handle's scratch slots.
 */
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <shared_mutex>

#include "awfm_score_affine_kernel.h"

extern "C" {

enum AwFmReturnCode awfmGpuScoreChainsAffine(AwFmGpuIndex *g, const struct AwFmVerifyInputs *dIn, uint64_t numReads, uint32_t maxCandidates,
                                             uint32_t bandPad, uint32_t maxDrift, const struct AwFmAlignScoring *scoring, uint32_t minScore,
                                             uint32_t mapqCap, const struct AwFmSlotScoreOutputs *dOut, void *stream) {
  if (!g) {
    setError("awfmGpuScoreChainsAffine: null image");
    return AwFmNullPtrError;
  }
  if (numReads == 0) return AwFmSuccess;
  if (!dIn || !dOut || !scoring || !dIn->readOffsets || !dIn->sequences || !dIn->chainAnchors || !dIn->chainReadBegins || !dIn->chainReadEnds ||
      !dIn->chainBeginDiagonals || !dIn->chainEndDiagonals || (!dIn->readChars && dIn->numReadChars != 0)) {
    setError("awfmGpuScoreChainsAffine: null argument");
    return AwFmNullPtrError;
  }
  if (numReads >= (1ull << 32) || maxCandidates < 1 || maxCandidates > AWFM_CANDIDATES_MAX_SLOTS) {
    setError("awfmGpuScoreChainsAffine: read numbers are 32-bit, and a read has 1 to 16 slots");
    return AwFmIllegalPositionError;
  }
  const uint64_t band = (uint64_t)maxDrift + 2ull * bandPad + 1ull;
  if (band > AWFM_VERIFY_MAX_BAND) {
    setError("awfmGpuScoreChainsAffine: the band, maxDrift + 2 bandPad + 1 diagonals, holds 64 at the most");
    return AwFmIllegalPositionError;
  }
  if (mapqCap > AWFM_SCORE_MAX_MAPQ) {
    setError("awfmGpuScoreChainsAffine: mapqCap is 0 to 254");
    return AwFmIllegalPositionError;
  }
  if (scoring->match < 1 || scoring->match > 255 || scoring->mismatch > 255 || scoring->gapOpen > 255 || scoring->gapExtend < 1 ||
      scoring->gapExtend > 255) {
    setError("awfmGpuScoreChainsAffine: match and gapExtend are 1 to 255, mismatch and gapOpen 0 to 255");
    return AwFmIllegalPositionError;
  }
  DeviceGuard guard(g->device);
  AwFmGpuImage *image = g->image;
  std::shared_lock<std::shared_mutex> lock(image->recordMutex); /* neither text nor record table is replaced before the launch */
  if (!image->dText) {
    setError("awfmGpuScoreChainsAffine: the image has no text (awfmGpuIndexSetText uploads it)");
    return AwFmUnsupportedVersionError;
  }
  DevScoreParams p{};
  p.in = *dIn;
  p.out = *dOut;
  p.text = (const unsigned char *)image->dText;
  p.length = image->textLength;
  p.ends = image->records.ends;
  p.numRecords = image->records.numRecords;
  p.numReads = numReads;
  p.slots = maxCandidates;
  p.pad = bandPad;
  p.drift = maxDrift;
  p.amino = g->amino ? 1u : 0u;
  p.floor = minScore > 1u ? minScore : 1u;
  p.cap = mapqCap;
  p.match = (int)scoring->match;
  p.mismatch = (int)scoring->mismatch;
  p.open = (int)(scoring->gapOpen + scoring->gapExtend);
  p.extend = (int)scoring->gapExtend;
  unsigned group = band <= 16u ? 16u : band <= 32u ? 32u : 64u;
  if (const char *env = awfmGpuDiag("score_group")) { /* tests: more lanes per slot than the band needs */
    const unsigned forced = (unsigned)atoi(env);
    if ((forced == 32u || forced == 64u) && forced > group) group = forced;
  }
  /* persistent grid over reads, a wave each */
  const uint64_t perBlock = kScoreThreads / 64u, blocks = (numReads + perBlock - 1u) / perBlock;
  const uint64_t resident = (uint64_t)g->numCUs * kScoreBlocksPerCU;
  const dim3 grid((unsigned)(blocks < resident ? blocks : resident)), block(kScoreThreads);
  hipStream_t s = (hipStream_t)stream;
  if (group == 16u) hipLaunchKernelGGL(scoreChainsAffineKernel<16>, grid, block, 0, s, p);
  else if (group == 32u) hipLaunchKernelGGL(scoreChainsAffineKernel<32>, grid, block, 0, s, p);
  else hipLaunchKernelGGL(scoreChainsAffineKernel<64>, grid, block, 0, s, p);
  AWFM_HIP_TRY(hipGetLastError(), AwFmGeneralFailure);
  return AwFmSuccess;
}

}  // extern "C"
