/*
 * awfm_gpu_records.hip -- the record table of a multi-record index in its device image, and the pass that maps located hits to
 * (sequence number, position in that sequence) on the device: awfmGpuIndexSetRecordTable, awfmGpuIndexNumRecords,
 * awfmGpuLocalPositions, awfmGpuLocateHostLocal (include/awfm_gpu.h).  The kernel is awfm_records_kernel.h.
 * ref src/AwFmSearch.c:284-301 (awFmGetLocalSequencePositionFromIndexPosition: one position per call, on the host).
 */
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <vector>

#include "awfm_records_kernel.h"

namespace {

/* log2 of the positions per directory bucket.  LDS lookup: the fewest positions that keep the directory within
 * kRecordLdsMaxBuckets (a genome's 3 * 10^9 positions: buckets of 2^20, a few records each at the most).  Lookup from memory: a
 * bucket no longer than the average record, so that it holds O(1) record ends on average and the directory has fewer than two
 * entries per record (360-residue records: buckets of 256 positions). */
unsigned chooseShift(uint64_t lastEnd, uint64_t numRecords, bool lds) {
  unsigned shift = 0;
  if (lds) {
    while (shift < 63u && ((lastEnd ? lastEnd - 1u : 0u) >> shift) + 1u > kRecordLdsMaxBuckets) shift++;
    return shift;
  }
  const uint64_t average = lastEnd / (numRecords ? numRecords : 1u);
  while (shift < 62u && (2ull << shift) <= average) shift++;
  return shift;
}

}  // namespace

enum AwFmReturnCode awfmGpuInstallRecordTable(AwFmGpuIndex *g, const uint64_t *ends, uint64_t numRecords) {
  AwFmGpuImage *image = g->image;
  DevRecords view{};
  void *dNew = nullptr;
  uint64_t bytes = 0;
  bool lds = false;
  unsigned ldsBytes = 0, grid = 0;
  DeviceGuard guard(g->device);
  if (numRecords != 0) {
    if (!ends) {
      setError("awfmGpuIndexSetRecordTable: null table");
      return AwFmNullPtrError;
    }
    if (numRecords >= 0xFFFFFFFFull) {
      setError("awfmGpuIndexSetRecordTable: sequence numbers are 32-bit (at most 2^32 - 2 records)");
      return AwFmIllegalPositionError;
    }
    /* E[r] >= S[r]: non-decreasing, and a record after another lies beyond that one's terminator */
    for (uint64_t r = 0; r < numRecords; r++)
      if (ends[r] >= (1ull << 62) || (r != 0 && ends[r] <= ends[r - 1])) {
        setError("awfmGpuIndexSetRecordTable: the records' ends must increase (every record ends with a terminator of its own) and lie below 2^62");
        return AwFmIllegalPositionError;
      }
    const uint64_t lastEnd = ends[numRecords - 1];
    lds = numRecords <= kRecordLdsMaxRecords;
    if (const char *env = awfmGpuDiag("record_lookup")) { /* tests: either lookup on the same table (lds only where it fits) */
      if (!strcmp(env, "dir")) lds = false;
    }
    const unsigned shift = chooseShift(lastEnd, numRecords, lds);
    const uint64_t numBuckets = ((lastEnd ? lastEnd - 1u : 0u) >> shift) + 1u;
    std::vector<unsigned> dir(numBuckets + 1u);
    uint64_t r = 0;
    for (uint64_t b = 0; b <= numBuckets; b++) { /* first record whose end lies beyond the bucket's start */
      while (r < numRecords && ends[r] <= (b << shift)) r++;
      dir[b] = (unsigned)r;
    }
    const uint64_t endsBytes = alignUp(numRecords * 8u, 16), dirBytes = alignUp((numBuckets + 1u) * 4u, 16);
    bytes = endsBytes + dirBytes;
    AWFM_HIP_TRY(hipMalloc(&dNew, bytes), AwFmAllocationFailure);
    hipError_t e = hipMemcpy(dNew, ends, numRecords * 8u, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy((uint8_t *)dNew + endsBytes, dir.data(), (numBuckets + 1u) * 4u, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      setError("awfmGpuIndexSetRecordTable: upload of the record table failed", e);
      (void)hipFree(dNew);
      return AwFmGeneralFailure;
    }
    view.ends = (const unsigned long long *)dNew;
    view.dir = (const unsigned *)((const uint8_t *)dNew + endsBytes);
    view.lastEnd = lastEnd;
    view.numRecords = (unsigned)numRecords;
    view.numBuckets = (unsigned)numBuckets;
    view.shift = shift;
    /* the persistent grid of this table's kernel: what is resident with its LDS */
    ldsBytes = lds ? (unsigned)(numRecords * 8u + (numBuckets + 1u) * 4u) : 0u;
    int perCU = 0;
    const hipError_t occ = lds ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, localPositionsKernel<true>, (int)kRecordThreads, ldsBytes)
                               : hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, localPositionsKernel<false>, (int)kRecordThreads, 0);
    if (occ != hipSuccess || perCU < 1) {
      (void)hipGetLastError();
      perCU = 2;
    }
    grid = (unsigned)g->numCUs * (unsigned)(perCU > 4 ? 4 : perCU);
  }
  void *dOld = nullptr;
  {
    std::unique_lock<std::shared_mutex> lock(image->recordMutex);
    dOld = image->dRecords;
    image->dRecords = dNew;
    image->records = view;
    image->recordBytes = bytes;
    image->recordsInLds = lds;
    image->recordLdsBytes = ldsBytes;
    image->recordGrid = grid;
  }
  if (dOld) (void)hipFree(dOld); /* waits for the mapping kernels that were enqueued with the old arrays */
  return AwFmSuccess;
}

enum AwFmReturnCode awfmGpuInstallRecordTableOf(AwFmGpuIndex *g, const struct AwFmIndex *index) {
  const struct FastaVector *fv = index->fastaVector;
  if (!fv || fv->numRecords == 0) return AwFmSuccess;
  std::vector<uint64_t> ends(fv->numRecords);
  for (size_t r = 0; r < fv->numRecords; r++) ends[r] = fv->records[r].sequenceEndPosition;
  return awfmGpuInstallRecordTable(g, ends.data(), ends.size());
}

std::string awfmGpuDescribeRecordTable(const AwFmGpuImage *image) {
  if (!image->records.numRecords) return "";
  return "record table: " + std::to_string(image->records.numRecords) + " records, lookup " + (image->recordsInLds ? "lds" : "dir") + " (" +
         std::to_string(image->records.numBuckets) + " buckets of 2^" + std::to_string(image->records.shift) + " positions), " +
         std::to_string(image->recordBytes) + " bytes; ";
}

extern "C" {

enum AwFmReturnCode awfmGpuIndexSetRecordTable(AwFmGpuIndex *g, const uint64_t *sequenceEndPositions, uint64_t numRecords) {
  if (!g) {
    setError("awfmGpuIndexSetRecordTable: null image");
    return AwFmNullPtrError;
  }
  AwFmGpuExclusive section(g->image); /* like every other change of the image's view */
  return awfmGpuInstallRecordTable(g, sequenceEndPositions, numRecords);
}

uint32_t awfmGpuIndexNumRecords(const AwFmGpuIndex *g) {
  if (!g) return 0;
  std::shared_lock<std::shared_mutex> lock(g->image->recordMutex);
  return g->image->records.numRecords;
}

enum AwFmReturnCode awfmGpuLocalPositions(AwFmGpuIndex *g, const uint64_t *dPositions, uint64_t capacity, const uint64_t *dNumPositions,
                                          uint32_t *dSequenceNumbers, uint64_t *dLocalPositions, uint64_t *dNumIllegal, void *stream) {
  if (!g) {
    setError("awfmGpuLocalPositions: null image");
    return AwFmNullPtrError;
  }
  if (capacity != 0 && (!dPositions || !dSequenceNumbers || !dLocalPositions)) {
    setError("awfmGpuLocalPositions: null argument");
    return AwFmNullPtrError;
  }
  DeviceGuard guard(g->device);
  AwFmGpuImage *image = g->image;
  std::shared_lock<std::shared_mutex> lock(image->recordMutex); /* the table is not replaced between reading its view and the launch */
  if (!image->records.numRecords) {
    setError("awfmGpuLocalPositions: the image has no record table (an index without records: awfmGpuIndexSetRecordTable installs one)");
    return AwFmUnsupportedVersionError;
  }
  if (capacity == 0) return AwFmSuccess;
  /* the grid from the capacity, trimmed by the count on the device */
  const uint64_t tiles = (capacity + (uint64_t)kRecordThreads * kRecordPerLane - 1u) / ((uint64_t)kRecordThreads * kRecordPerLane);
  const unsigned grid = (unsigned)(tiles < image->recordGrid ? tiles : image->recordGrid);
  hipStream_t s = (hipStream_t)stream;
  if (image->recordsInLds)
    hipLaunchKernelGGL(localPositionsKernel<true>, dim3(grid), dim3(kRecordThreads), image->recordLdsBytes, s, image->records,
                       (const unsigned long long *)dPositions, (unsigned long long)capacity, (const unsigned long long *)dNumPositions,
                       (unsigned *)dSequenceNumbers, (unsigned long long *)dLocalPositions, (unsigned long long *)dNumIllegal);
  else
    hipLaunchKernelGGL(localPositionsKernel<false>, dim3(grid), dim3(kRecordThreads), 0, s, image->records,
                       (const unsigned long long *)dPositions, (unsigned long long)capacity, (const unsigned long long *)dNumPositions,
                       (unsigned *)dSequenceNumbers, (unsigned long long *)dLocalPositions, (unsigned long long *)dNumIllegal);
  AWFM_HIP_TRY(hipGetLastError(), AwFmGeneralFailure);
  return AwFmSuccess;
}

namespace {
struct LocalSinkCtx {
  uint64_t *hitOffsets, n;
  uint32_t *seq;
  uint64_t *local;
  const uint32_t *seqOfWindow; /* set by the windowed locate before every sink call */
  bool failed;
};
int localSink(void *user, uint64_t, uint64_t, uint64_t hitBegin, uint64_t hitEnd, const uint64_t *positions) {
  LocalSinkCtx *z = (LocalSinkCtx *)user;
  if (!z->local) { /* the flat arrays need the total first: allocated on the first window */
    const uint64_t total = z->hitOffsets[z->n] ? z->hitOffsets[z->n] : 1;
    z->seq = (uint32_t *)malloc(total * 4);
    z->local = (uint64_t *)malloc(total * 8);
    if (!z->seq || !z->local) {
      z->failed = true;
      return 1;
    }
  }
  memcpy(z->local + hitBegin, positions, (hitEnd - hitBegin) * 8);
  memcpy(z->seq + hitBegin, z->seqOfWindow, (hitEnd - hitBegin) * 4);
  return 0;
}
}  // namespace

enum AwFmReturnCode awfmGpuLocateHostLocal(AwFmGpuIndex *g, const uint8_t *chars, const uint64_t *offsets, uint32_t fixedLength,
                                           uint64_t numQueries, struct AwFmSearchRange *ranges, uint64_t *hitOffsets,
                                           uint32_t **sequenceNumbers, uint64_t **localPositions, uint64_t *numIllegal) {
  if (!g || !sequenceNumbers || !localPositions) {
    setError("awfmGpuLocateHostLocal: null argument");
    return AwFmNullPtrError;
  }
  *sequenceNumbers = nullptr;
  *localPositions = nullptr;
  if (numIllegal) *numIllegal = 0;
  if (awfmGpuIndexNumRecords(g) == 0) {
    setError("awfmGpuLocateHostLocal: the image has no record table (an index without records: awfmGpuIndexSetRecordTable installs one)");
    return AwFmUnsupportedVersionError;
  }
  LocalSinkCtx ctx = {hitOffsets, numQueries, nullptr, nullptr, nullptr, false};
  uint64_t illegal = 0;
  const enum AwFmReturnCode rc = awfmGpuLocateHostWindowsMapped(g, chars, offsets, fixedLength, numQueries, ranges, hitOffsets, localSink, &ctx,
                                                                &ctx.seqOfWindow, &illegal);
  if (rc != AwFmSuccess || ctx.failed) {
    free(ctx.seq);
    free(ctx.local);
    if (ctx.failed) setError("awfmGpuLocateHostLocal: host allocation failed");
    return ctx.failed ? AwFmAllocationFailure : rc;
  }
  if (!ctx.local) { /* no hits: empty arrays the caller can free */
    ctx.seq = (uint32_t *)malloc(4);
    ctx.local = (uint64_t *)malloc(8);
  }
  *sequenceNumbers = ctx.seq;
  *localPositions = ctx.local;
  if (numIllegal) *numIllegal = illegal;
  return AwFmSuccess;
}

}  // extern "C"
