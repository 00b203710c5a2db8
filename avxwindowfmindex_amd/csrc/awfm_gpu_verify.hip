/*
 * awfm_gpu_verify.hip -- "chain verification" on the device (include/awfm_gpu.h): the indexed text in the device image
 * (awfmGpuIndexSetText, awfmGpuIndexTextLength), its batched recall (awfmGpuTextWindows) and the banded edit distance of every
 * chain slot (awfmGpuVerifyChains).  The kernels are awfm_verify_kernel.h, the host twins and checkers awfm_verify.c.
 * ref src/AwFmFile.c (awFmReadSequenceFromFile: one segment of the stored text per call, on the host).
 */
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <shared_mutex>
#include <string>

#include "awfm_verify_kernel.h"

/* The text is published under the record table's leaf lock (AwFmGpuImage::recordMutex): a verification reads both views at
 * once. */
enum AwFmReturnCode awfmGpuInstallText(AwFmGpuIndex *g, const uint8_t *text, uint64_t length) {
  AwFmGpuImage *image = g->image;
  void *dNew = nullptr;
  uint64_t bytes = 0;
  DeviceGuard guard(g->device);
  if (length != 0) {
    if (!text) {
      setError("awfmGpuIndexSetText: null text");
      return AwFmNullPtrError;
    }
    if (length != image->dev.bwtLength - 1ull) {
      setError("awfmGpuIndexSetText: the text of an image is bwtLength - 1 bytes long");
      return AwFmIllegalPositionError;
    }
    /* the zeros behind the text: an aligned load of up to 16 bytes that holds one of its bytes stays inside */
    bytes = alignUp(length, 16) + 16u;
    AWFM_HIP_TRY(hipMalloc(&dNew, bytes), AwFmAllocationFailure);
    const uint64_t tailAt = length & ~15ull;
    hipError_t e = hipMemset((uint8_t *)dNew + tailAt, 0, bytes - tailAt);
    if (e == hipSuccess) e = hipMemcpy(dNew, text, length, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      setError("awfmGpuIndexSetText: upload of the text failed", e);
      (void)hipFree(dNew);
      return AwFmGeneralFailure;
    }
  }
  void *dOld = nullptr;
  {
    std::unique_lock<std::shared_mutex> lock(image->recordMutex);
    dOld = image->dText;
    image->dText = dNew;
    image->textLength = length;
    image->textBytes = bytes;
  }
  if (dOld) (void)hipFree(dOld); /* waits for the kernels that were enqueued with the old text */
  return AwFmSuccess;
}

std::string awfmGpuDescribeText(const AwFmGpuImage *image) {
  if (!image->textLength) return "";
  return "text: " + std::to_string(image->textLength) + " positions, " + std::to_string(image->textBytes) + " bytes; ";
}

extern "C" {

enum AwFmReturnCode awfmGpuIndexSetText(AwFmGpuIndex *g, const uint8_t *text, uint64_t length) {
  if (!g) {
    setError("awfmGpuIndexSetText: null image");
    return AwFmNullPtrError;
  }
  AwFmGpuExclusive section(g->image); /* like every other change of the image's view */
  return awfmGpuInstallText(g, text, text ? length : 0);
}

uint64_t awfmGpuIndexTextLength(const AwFmGpuIndex *g) {
  if (!g) return 0;
  std::shared_lock<std::shared_mutex> lock(g->image->recordMutex);
  return g->image->textLength;
}

enum AwFmReturnCode awfmGpuTextWindows(AwFmGpuIndex *g, const uint64_t *dPositions, uint64_t capacity, const uint64_t *dNumPositions,
                                       uint32_t before, uint32_t after, uint8_t *dOut, void *stream) {
  if (!g) {
    setError("awfmGpuTextWindows: null image");
    return AwFmNullPtrError;
  }
  const uint64_t width = (uint64_t)before + after;
  if (width < 1 || width > 4096) {
    setError("awfmGpuTextWindows: a window is 1 to 4096 bytes wide");
    return AwFmIllegalPositionError;
  }
  if (capacity != 0 && (!dPositions || !dOut)) {
    setError("awfmGpuTextWindows: null argument");
    return AwFmNullPtrError;
  }
  DeviceGuard guard(g->device);
  AwFmGpuImage *image = g->image;
  std::shared_lock<std::shared_mutex> lock(image->recordMutex); /* the text is not replaced between reading its view and the launch */
  if (textMissing("awfmGpuTextWindows", image) != AwFmSuccess) return AwFmUnsupportedVersionError;
  if (capacity == 0) return AwFmSuccess;
  /* the grid from the capacity (a thread per output dword), trimmed by the count on the device */
  const uint64_t blocks = (capacity * width / 4u + 2u + kWindowThreads - 1u) / kWindowThreads, resident = (uint64_t)g->numCUs * 8u;
  hipLaunchKernelGGL(textWindowsKernel, dim3((unsigned)(blocks < resident ? blocks : resident)), dim3(kWindowThreads), 0, (hipStream_t)stream,
                     (const unsigned char *)image->dText, (unsigned long long)image->textLength, (const unsigned long long *)dPositions,
                     (unsigned long long)capacity, (const unsigned long long *)dNumPositions, (unsigned)before, (unsigned)width,
                     (unsigned char *)dOut);
  AWFM_HIP_TRY(hipGetLastError(), AwFmGeneralFailure);
  return AwFmSuccess;
}

enum AwFmReturnCode awfmGpuVerifyChains(AwFmGpuIndex *g, const struct AwFmVerifyInputs *dIn, uint64_t numReads, uint32_t maxCandidates,
                                        uint32_t bandPad, uint32_t maxDrift, const struct AwFmVerifyOutputs *dOut, void *stream) {
  if (!g) {
    setError("awfmGpuVerifyChains: null image");
    return AwFmNullPtrError;
  }
  if (numReads == 0) return AwFmSuccess;
  const char *name = "awfmGpuVerifyChains";
  const uint64_t band = (uint64_t)maxDrift + 2ull * bandPad + 1ull;
  enum AwFmReturnCode rc = chainArgumentsRefused(name, dIn, dOut != nullptr, numReads, maxCandidates, band);
  if (rc != AwFmSuccess) return rc;
  DeviceGuard guard(g->device);
  AwFmGpuImage *image = g->image;
  std::shared_lock<std::shared_mutex> lock(image->recordMutex); /* neither text nor record table is replaced before the launch */
  if ((rc = textMissing(name, image)) != AwFmSuccess) return rc;
  DevVerifyParams p{};
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
  const unsigned group = bandGroup(band, "verify_group");
  /* persistent grid over reads, a wave each: the six workgroups of four waves per CU that the kernel's registers leave room for */
  const uint64_t waves = kVerifyThreads / 64u, blocks = (numReads + waves - 1u) / waves, resident = (uint64_t)g->numCUs * kVerifyBlocksPerCU;
  const dim3 grid((unsigned)(blocks < resident ? blocks : resident)), block(kVerifyThreads);
  AWFM_LAUNCH_BAND_KERNEL(verifyChainsKernel, group, grid, block, stream, p);
  AWFM_HIP_TRY(hipGetLastError(), AwFmGeneralFailure);
  return AwFmSuccess;
}

}  // extern "C"
