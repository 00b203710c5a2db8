/*
 * awfm_records_kernel.h -- global text position -> (record, position inside the record) for a batch of located hits:
 * the device form of awFmGetLocalSequencePositionFromIndexPosition (ref src/AwFmSearch.c:284-301) over the image's record
 * table (DevRecords, awfm_device.h).
 *
 * With ends E[0..R) and starts S[0] = 0, S[r] = E[r-1] + 1, position p belongs to the first r with E[r] > p when p >= S[r];
 * otherwise (p is a record's terminator, or p >= E[R-1]) it is illegal: sequence 0xFFFFFFFF, position kept, counted.  Empty
 * records (E[r] == S[r]) own no position and fall out of that definition by themselves.
 *
 * The pass streams 8 bytes in and 12 bytes out per position; the search in the middle must not turn it into a gather.  The
 * directory gives the record's candidates from one read -- dir[p >> shift] .. dir[(p >> shift) + 1], an interval that holds
 * O(1) records for a table of ordinary records -- and a binary search over that interval ends it: no read for an interval
 * of one record, one for two, and log2 of them for a bucket into which a run of empty or one-residue records falls (bounded by
 * log2 R whatever the table looks like).  One more read gives the start.
 *
 *   LDS = true   tables of up to kRecordLdsMaxRecords records with a directory of up to kRecordLdsMaxBuckets buckets (a genome):
 *                ends and directory are staged into dynamic LDS once per workgroup of a persistent grid (48 KB at most: three
 *                workgroups per CU), the reads are ds_read_b64 / ds_read_b32 of unrelated addresses, i.e. a few bank conflicts
 *                each and no traffic beyond the stream.
 *   LDS = false  any table (a protein set: 5.7 * 10^5 records are 4.6 MB of ends and as much directory): the same reads from
 *                memory; both arrays stay in the L2s / the Infinity Cache, the stream does not.
 *
 * Vector loads and stores only; positions are 64-bit whatever the image's width (the pass is bound by the 8-byte positions
 * either way).
 */
#ifndef AWFM_RECORDS_KERNEL_H
#define AWFM_RECORDS_KERNEL_H

#include "awfm_device.h"

namespace {

constexpr unsigned kRecordThreads = 512;         /* per workgroup */
constexpr unsigned kRecordPerLane = 4;           /* positions a lane has in flight per round */
constexpr unsigned kRecordLdsMaxRecords = 4096;  /* 32 KB of ends ... */
constexpr unsigned kRecordLdsMaxBuckets = 4096;  /* ... and 16 KB of directory: 48 KB + 4 B of LDS per workgroup at most */
constexpr unsigned kRecordIllegal = 0xFFFFFFFFu;

/* the record of position p (p < lastEnd) from the two arrays, wherever they are */
__device__ __forceinline__ unsigned recordOf(const unsigned long long *__restrict__ ends, const unsigned *__restrict__ dir, unsigned shift,
                                             unsigned lastRecord, unsigned long long p) {
  const unsigned bucket = (unsigned)(p >> shift);
  unsigned lo = dir[bucket], hi = dir[bucket + 1u];
  hi = hi < lastRecord ? hi : lastRecord; /* (p < lastEnd: the last record's end is beyond it) */
  while (lo < hi) {                       /* first record of [lo, hi] whose end is beyond p */
    const unsigned mid = (lo + hi) >> 1;
    const bool beyond = ends[mid] > p;
    hi = beyond ? mid : hi;
    lo = beyond ? lo : mid + 1u;
  }
  return lo;
}

template <bool LDS>
__global__ void __launch_bounds__(kRecordThreads)
localPositionsKernel(const DevRecords rec, const unsigned long long *positions, const unsigned long long capacity,
                     const unsigned long long *__restrict__ numOnDevice, unsigned *__restrict__ sequenceNumbers,
                     unsigned long long *localPositions /* may be `positions` */, unsigned long long *__restrict__ numIllegal) {
  extern __shared__ unsigned long long sRecords[]; /* LDS: ends[numRecords], then dir[numBuckets + 1] */
  const unsigned long long *ends = rec.ends;
  const unsigned *dir = rec.dir;
  if (LDS) {
    unsigned *sDir = (unsigned *)(sRecords + rec.numRecords);
    for (unsigned e = threadIdx.x; e < rec.numRecords; e += kRecordThreads) sRecords[e] = rec.ends[e];
    for (unsigned e = threadIdx.x; e <= rec.numBuckets; e += kRecordThreads) sDir[e] = rec.dir[e];
    __syncthreads();
    ends = sRecords;
    dir = sDir;
  }
  unsigned long long n = capacity;
  if (numOnDevice) {
    const unsigned long long have = *numOnDevice;
    n = have < n ? have : n;
  }
  const unsigned lastRecord = rec.numRecords - 1u;
  unsigned illegal = 0;
  constexpr unsigned long long kTile = (unsigned long long)kRecordThreads * kRecordPerLane;
  for (unsigned long long tile = (unsigned long long)blockIdx.x * kTile; tile < n; tile += (unsigned long long)gridDim.x * kTile) {
    unsigned long long p[kRecordPerLane]; /* the round's reads of the stream are issued before the first search */
#pragma unroll
    for (unsigned k = 0; k < kRecordPerLane; k++) {
      const unsigned long long i = tile + k * kRecordThreads + threadIdx.x;
      p[k] = i < n ? positions[i] : ~0ull;
    }
#pragma unroll
    for (unsigned k = 0; k < kRecordPerLane; k++) {
      const unsigned long long i = tile + k * kRecordThreads + threadIdx.x;
      if (i >= n) continue;
      unsigned sequence = kRecordIllegal;
      unsigned long long local = p[k];
      if (p[k] < rec.lastEnd) {
        const unsigned r = recordOf(ends, dir, rec.shift, lastRecord, p[k]);
        const unsigned long long start = r ? ends[r - 1u] + 1ull : 0ull;
        if (p[k] >= start) { /* (below it: the terminator of the record before) */
          sequence = r;
          local = p[k] - start;
        }
      }
      illegal += sequence == kRecordIllegal ? 1u : 0u;
      sequenceNumbers[i] = sequence;
      localPositions[i] = local;
    }
  }
  if (numIllegal) { /* one atomic per wave that met any */
#pragma unroll
    for (int offset = 32; offset > 0; offset >>= 1) illegal += (unsigned)__shfl_xor((int)illegal, offset, 64);
    if ((threadIdx.x & 63u) == 0u && illegal) atomicAdd(numIllegal, (unsigned long long)illegal);
  }
}

}  // namespace

#endif
