/*
 * awfm_gpu_sam.hip -- "SAM records" on the device (include/awfm_gpu.h): awfmGpuSamRecords and the size of its scratch.  The
 * kernels are awfm_sam_kernel.h, the host twin and checker awfm_sam.c.  On the caller's stream: one launch for the lengths, the
 * library's scan (awfm_gpu_locate.hip: one to three launches by the batch's size) when the offsets are asked for, one launch for
 * the bytes when the arena is; none of the handle's scratch slots, neither the image's text nor its record table.
 */
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>

#include "awfm_sam_kernel.h"

namespace {

/* the scratch: the line lengths (32 bits a read, rounded up to 256 bytes), then the scan's */
uint64_t samLengthBytes(uint64_t numReads) { return (numReads * 4u + 255u) & ~(uint64_t)255u; }

}  // namespace

extern "C" {

uint64_t awfmGpuSamRecordsScratchBytes(const AwFmGpuIndex *g, uint64_t numReads) {
  if (!g || numReads == 0 || numReads >= (1ull << 32)) return 0;
  return samLengthBytes(numReads) + awfmGpuScanScratchBytes(numReads);
}

enum AwFmReturnCode awfmGpuSamRecords(AwFmGpuIndex *g, const struct AwFmSamInputs *dIn, uint64_t numReads, uint32_t maxCandidates,
                                      uint32_t flags, const struct AwFmSamOutputs *dOut, void *dScratch, void *stream) {
  if (!g) {
    setError("awfmGpuSamRecords: null image");
    return AwFmNullPtrError;
  }
  if (numReads == 0) return AwFmSuccess;
  if (!dIn || !dOut || !dScratch || !dIn->readChars || !dIn->readOffsets || !dIn->sequences || !dIn->slots || !dIn->scores ||
      !dIn->editDistances || !dIn->textBegins || !dIn->textEnds || !dIn->cigarOffsets || !dIn->cigarChars ||
      (dIn->numRecordNames != 0 && (!dIn->recordNameOffsets || !dIn->recordNameChars))) {
    setError("awfmGpuSamRecords: null argument");
    return AwFmNullPtrError;
  }
  if (!dIn->nameOffsets != !dIn->nameChars || !dIn->mdOffsets != !dIn->mdChars) {
    setError("awfmGpuSamRecords: names and MD strings come as offsets and arena, or not at all");
    return AwFmNullPtrError;
  }
  if (dOut->lineChars && !dOut->lineOffsets) {
    setError("awfmGpuSamRecords: an arena needs its offsets array");
    return AwFmNullPtrError;
  }
  if (maxCandidates < 1 || maxCandidates > AWFM_CANDIDATES_MAX_SLOTS || (flags & ~AWFM_SAM_PAIRED)) {
    setError("awfmGpuSamRecords: a read has 1 to 16 slots, flags 0 or AWFM_SAM_PAIRED");
    return AwFmIllegalPositionError;
  }
  if (((flags & AWFM_SAM_PAIRED) && (numReads & 1u)) || numReads >= (1ull << 32)) {
    setError("awfmGpuSamRecords: mates come in twos, and read numbers are 32-bit");
    return AwFmIllegalPositionError;
  }
  if ((uintptr_t)dScratch & 15u) {
    setError("awfmGpuSamRecords: the scratch is aligned to 16 bytes");
    return AwFmIllegalPositionError;
  }
  DeviceGuard guard(g->device);
  DevSamParams p{};
  p.in = *dIn;
  p.out = *dOut;
  p.numReads = numReads;
  p.lengths = (unsigned *)dScratch;
  p.slots = maxCandidates;
  p.paired = (flags & AWFM_SAM_PAIRED) ? 1u : 0u;
  if (const char *env = awfmGpuDiag("sam_tier")) { /* tests: every line straight to the arena, where it would fit the tile */
    if (!strcmp(env, "direct")) p.direct = 1u;
  }
  void *scanScratch = (unsigned char *)dScratch + samLengthBytes(numReads);
  hipStream_t s = (hipStream_t)stream;
  const dim3 lengthsGrid((unsigned)((numReads + kSamThreads - 1u) / kSamThreads)), block(kSamThreads);
  hipLaunchKernelGGL(samLengthsKernel, lengthsGrid, block, 0, s, p);
  AWFM_HIP_TRY(hipGetLastError(), AwFmGeneralFailure);
  if (!dOut->lineOffsets) return AwFmSuccess; /* the counter alone */
  enum AwFmReturnCode rc = awfmGpuScanCounts(g, p.lengths, numReads, dOut->lineOffsets, scanScratch, s);
  if (rc != AwFmSuccess) return rc;
  if (!dOut->lineChars) return AwFmSuccess; /* offsets only: how a caller sizes the arena */
  constexpr unsigned kSamWaves = kSamThreads / 64u; /* a wave a read: below 2^30 workgroups */
  const dim3 writeGrid((unsigned)((numReads + kSamWaves - 1u) / kSamWaves));
  hipLaunchKernelGGL(samWriteKernel, writeGrid, block, 0, s, p);
  AWFM_HIP_TRY(hipGetLastError(), AwFmGeneralFailure);
  return AwFmSuccess;
}

}  // extern "C"
