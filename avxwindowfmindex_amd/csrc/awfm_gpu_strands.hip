/*
 * awfm_gpu_strands.hip -- "strands" on the device (include/awfm_gpu.h): awfmGpuChooseStrands and awfmGpuOrientReads.
 * The kernels are awfm_strands_kernel.h, the host twins and checkers awfm_strands.c.  One launch each, no scratch, none of the
 * handle's scratch slots, nothing of the image but its device.
 */
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "awfm_strands_kernel.h"

extern "C" {

enum AwFmReturnCode awfmGpuChooseStrands(AwFmGpuIndex *g, const struct AwFmStrandInputs *dIn, uint64_t numReads, uint32_t maxCandidates,
                                         uint32_t flags, const struct AwFmPairParams *params, const struct AwFmStrandOutputs *dOut,
                                         void *stream) {
  if (!g) {
    setError("awfmGpuChooseStrands: null image");
    return AwFmNullPtrError;
  }
  if (numReads == 0) return AwFmSuccess;
  if (!dIn || !dOut || !params || !dIn->readOffsets || !dIn->sequences || !dIn->slotScores || !dIn->slotReadEnds || !dIn->slotTextEnds) {
    setError("awfmGpuChooseStrands: null argument");
    return AwFmNullPtrError;
  }
  if (maxCandidates < 1 || maxCandidates > AWFM_CANDIDATES_MAX_SLOTS || numReads >= (1ull << 31)) {
    setError("awfmGpuChooseStrands: row numbers are 32-bit, and a row has 1 to 16 slots");
    return AwFmIllegalPositionError;
  }
  const bool paired = (flags & AWFM_STRANDS_PAIRED) != 0;
  if ((flags & ~AWFM_STRANDS_PAIRED) != 0 || (paired && (numReads & 1u))) {
    setError("awfmGpuChooseStrands: flags is 0 or AWFM_STRANDS_PAIRED, which wants an even number of reads");
    return AwFmIllegalPositionError;
  }
  if ((paired && (params->minInsert > params->maxInsert || params->minInsert < -AWFM_PAIR_MAX_INSERT || params->maxInsert > AWFM_PAIR_MAX_INSERT)) ||
      params->mapqCap > AWFM_SCORE_MAX_MAPQ) {
    setError("awfmGpuChooseStrands: minInsert <= maxInsert, both within 2^40 of 0, and mapqCap is 0 to 254");
    return AwFmIllegalPositionError;
  }
  DeviceGuard guard(g->device);
  DevStrandParams p{};
  p.in = *dIn;
  p.out = *dOut;
  p.numReads = numReads;
  p.minInsert = paired ? params->minInsert : 0;
  p.maxInsert = paired ? params->maxInsert : 0;
  p.pad = (long long)params->windowPad;
  p.slots = maxCandidates;
  p.floor = params->minScore > 1u ? params->minScore : 1u;
  p.penalty = params->unpairedPenalty;
  p.cap = params->mapqCap;
  unsigned group = paired ? (maxCandidates <= 4u ? 32u : 64u) : 16u;
  if (const char *env = awfmGpuDiag("strand_group")) { /* tests: a wave per pair or read where fewer lanes would do */
    if ((unsigned)atoi(env) == 64u) group = 64u;
  }
  /* persistent grid over pairs or reads, a group each */
  const uint64_t items = paired ? numReads / 2u : numReads, perBlock = kStrandThreads / group, blocks = (items + perBlock - 1u) / perBlock;
  const uint64_t resident = (uint64_t)g->numCUs * (paired && group == 64u ? kStrandWaveBlocksPerCU : kStrandBlocksPerCU);
  const dim3 grid((unsigned)(blocks < resident ? blocks : resident)), block(kStrandThreads);
  hipStream_t s = (hipStream_t)stream;
  if (paired && group == 32u) hipLaunchKernelGGL(chooseStrandPairsKernel<32>, grid, block, 0, s, p);
  else if (paired) hipLaunchKernelGGL(chooseStrandPairsKernel<64>, grid, block, 0, s, p);
  else if (group == 16u) hipLaunchKernelGGL(chooseStrandReadsKernel<16>, grid, block, 0, s, p);
  else hipLaunchKernelGGL(chooseStrandReadsKernel<64>, grid, block, 0, s, p);
  AWFM_HIP_TRY(hipGetLastError(), AwFmGeneralFailure);
  return AwFmSuccess;
}

static bool orientOverlap(const void *x, uint64_t xBytes, const void *y, uint64_t yBytes) {
  return x && y && xBytes && yBytes && (uintptr_t)x < (uintptr_t)y + yBytes && (uintptr_t)y < (uintptr_t)x + xBytes;
}

enum AwFmReturnCode awfmGpuOrientReads(AwFmGpuIndex *g, const struct AwFmOrientInputs *dIn, uint64_t numReads, uint32_t maxCandidates,
                                       const struct AwFmOrientOutputs *dOut, void *stream) {
  if (!g) {
    setError("awfmGpuOrientReads: null image");
    return AwFmNullPtrError;
  }
  if (numReads == 0) return AwFmSuccess;
  if (!dIn || !dOut || !dIn->rows.readOffsets || !dIn->strands || !dOut->readOffsets || (!dIn->rows.readChars && dIn->rows.numReadChars != 0) ||
      (!dOut->readChars && dOut->capacity != 0)) {
    setError("awfmGpuOrientReads: null argument");
    return AwFmNullPtrError;
  }
  if (!dIn->qualities != !dOut->qualities || !dIn->rows.sequences != !dOut->sequences || !dIn->rows.chainAnchors != !dOut->chainAnchors ||
      !dIn->rows.chainReadBegins != !dOut->chainReadBegins || !dIn->rows.chainReadEnds != !dOut->chainReadEnds ||
      !dIn->rows.chainBeginDiagonals != !dOut->chainBeginDiagonals || !dIn->rows.chainEndDiagonals != !dOut->chainEndDiagonals ||
      !dIn->slotScores != !dOut->slotScores || !dIn->slotReadEnds != !dOut->slotReadEnds || !dIn->slotTextEnds != !dOut->slotTextEnds) {
    setError("awfmGpuOrientReads: an output is given exactly when its input is");
    return AwFmNullPtrError;
  }
  if (maxCandidates < 1 || maxCandidates > AWFM_CANDIDATES_MAX_SLOTS || numReads >= (1ull << 31)) {
    setError("awfmGpuOrientReads: row numbers are 32-bit, and a row has 1 to 16 slots");
    return AwFmIllegalPositionError;
  }
  if (orientOverlap(dIn->rows.readChars, dIn->rows.numReadChars, dOut->readChars, dOut->capacity) ||
      orientOverlap(dIn->qualities, dIn->rows.numReadChars, dOut->qualities, dOut->capacity)) {
    setError("awfmGpuOrientReads: input and output overlap");
    return AwFmIllegalPositionError;
  }
  DeviceGuard guard(g->device);
  DevOrientParams p{};
  p.in = *dIn;
  p.out = *dOut;
  p.numReads = numReads;
  p.slots = maxCandidates;
  /* persistent grid over reads, a wave each */
  const uint64_t perBlock = kOrientThreads / 64u, blocks = (numReads + perBlock - 1u) / perBlock;
  const uint64_t resident = (uint64_t)g->numCUs * kOrientBlocksPerCU;
  const dim3 grid((unsigned)(blocks < resident ? blocks : resident)), block(kOrientThreads);
  hipLaunchKernelGGL(orientReadsKernel, grid, block, 0, (hipStream_t)stream, p);
  AWFM_HIP_TRY(hipGetLastError(), AwFmGeneralFailure);
  return AwFmSuccess;
}

}  // extern "C"
