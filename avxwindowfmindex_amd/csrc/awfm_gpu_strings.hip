/*
 * awfm_gpu_strings.hip -- "alignment strings" on the device (include/awfm_gpu.h): awfmGpuAlignmentStrings and the size of its
 * scratch.  The kernels are awfm_strings_kernel.h, the host twin and checker awfm_strings.c.  On the caller's stream: one
 * launch for the lengths, the library's scan (awfm_gpu_locate.hip: one to three launches by the batch's size, three at 2^20 reads) for
 * each offsets array asked for, one launch for the bytes -- eight at that size with both strings --; none of the handle's scratch slots.
 */
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <shared_mutex>

#include "awfm_strings_kernel.h"

namespace {

/* the scratch: the CIGAR lengths, the MD lengths (32 bits a read each, the pair rounded up to 256 bytes), then the scan's */
uint64_t stringsLengthBytes(uint64_t numReads) { return (numReads * 8u + 255u) & ~(uint64_t)255u; }

}  // namespace

extern "C" {

uint64_t awfmGpuAlignmentStringsScratchBytes(const AwFmGpuIndex *g, uint64_t numReads) {
  if (!g || numReads == 0 || numReads >= (1ull << 32)) return 0;
  return stringsLengthBytes(numReads) + awfmGpuScanScratchBytes(numReads);
}

enum AwFmReturnCode awfmGpuAlignmentStrings(AwFmGpuIndex *g, const struct AwFmStringInputs *dIn, uint64_t numReads, uint32_t maxCandidates,
                                            uint32_t maxOps, uint32_t flags, const struct AwFmStringOutputs *dOut, void *dScratch,
                                            void *stream) {
  if (!g) {
    setError("awfmGpuAlignmentStrings: null image");
    return AwFmNullPtrError;
  }
  if (numReads == 0) return AwFmSuccess;
  if (!dIn || !dOut || !dScratch || !dIn->sequences || !dIn->slots || !dIn->textBegins || !dIn->numOps || !dIn->ops) {
    setError("awfmGpuAlignmentStrings: null argument");
    return AwFmNullPtrError;
  }
  if ((dOut->cigarChars && !dOut->cigarOffsets) || (dOut->mdChars && !dOut->mdOffsets)) {
    setError("awfmGpuAlignmentStrings: an arena needs its offsets array");
    return AwFmNullPtrError;
  }
  if (numReads >= (1ull << 32) || maxCandidates < 1 || maxCandidates > AWFM_CANDIDATES_MAX_SLOTS) {
    setError("awfmGpuAlignmentStrings: read numbers are 32-bit, and a read has 1 to 16 slots");
    return AwFmIllegalPositionError;
  }
  if (maxOps < 1 || maxOps > AWFM_ALIGN_MAX_OPS || (flags & ~AWFM_STRINGS_CIGAR_M)) {
    setError("awfmGpuAlignmentStrings: maxOps is 1 to 4096, flags 0 or AWFM_STRINGS_CIGAR_M");
    return AwFmIllegalPositionError;
  }
  if ((uintptr_t)dScratch & 15u) {
    setError("awfmGpuAlignmentStrings: the scratch is aligned to 16 bytes");
    return AwFmIllegalPositionError;
  }
  DeviceGuard guard(g->device);
  AwFmGpuImage *image = g->image;
  std::shared_lock<std::shared_mutex> lock(image->recordMutex); /* neither text nor record table is replaced before the launches */
  if (!image->dText) {
    setError("awfmGpuAlignmentStrings: the image has no text (awfmGpuIndexSetText uploads it)");
    return AwFmUnsupportedVersionError;
  }
  DevStringParams p{};
  p.in = *dIn;
  p.out = *dOut;
  p.text = (const unsigned char *)image->dText;
  p.ends = image->records.ends;
  p.length = image->textLength;
  p.numReads = numReads;
  p.cigarLengths = (unsigned *)dScratch;
  p.mdLengths = p.cigarLengths + numReads;
  p.numRecords = image->records.numRecords;
  p.slots = maxCandidates;
  p.maxOps = maxOps;
  p.classic = (flags & AWFM_STRINGS_CIGAR_M) ? 1u : 0u;
  p.amino = g->amino ? 1u : 0u;
  if (const char *env = awfmGpuDiag("strings_tier")) { /* tests: byte stores read by read where the span would fit the tile */
    if (!strcmp(env, "direct")) p.direct = 1u;
  }
  void *scanScratch = (unsigned char *)dScratch + stringsLengthBytes(numReads);
  /* a row is read in 16-byte loads when every row begins on a 16-byte boundary */
  const bool wide = maxOps % 4u == 0u && ((uintptr_t)dIn->ops & 15u) == 0u;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((numReads + kStringsThreads - 1u) / kStringsThreads)), block(kStringsThreads); /* < 2^24 workgroups */
  if (wide) hipLaunchKernelGGL(stringLengthsKernel<true>, grid, block, 0, s, p);
  else hipLaunchKernelGGL(stringLengthsKernel<false>, grid, block, 0, s, p);
  AWFM_HIP_TRY(hipGetLastError(), AwFmGeneralFailure);
  enum AwFmReturnCode rc = AwFmSuccess;
  if (dOut->cigarOffsets && (rc = awfmGpuScanCounts(g, p.cigarLengths, numReads, dOut->cigarOffsets, scanScratch, s)) != AwFmSuccess) return rc;
  if (dOut->mdOffsets && (rc = awfmGpuScanCounts(g, p.mdLengths, numReads, dOut->mdOffsets, scanScratch, s)) != AwFmSuccess) return rc;
  if (!dOut->cigarChars && !dOut->mdChars) return AwFmSuccess; /* offsets only: how a caller sizes an arena */
  if (wide) hipLaunchKernelGGL(stringWriteKernel<true>, grid, block, 0, s, p);
  else hipLaunchKernelGGL(stringWriteKernel<false>, grid, block, 0, s, p);
  AWFM_HIP_TRY(hipGetLastError(), AwFmGeneralFailure);
  return AwFmSuccess;
}

}  // extern "C"
