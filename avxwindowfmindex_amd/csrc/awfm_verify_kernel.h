/*
 * awfm_verify_kernel.h -- the kernels of "chain verification" (include/awfm_gpu.h): textWindowsKernel, the batched recall of the
 * image's text, and verifyChainsKernel<G>, the banded global edit distance of every chain slot against the text it names.  The
 * definition is the header's; the host twin and checker is awfm_verify.c.  The classification of a slot, the staging and the
 * letters are awfm_band_kernel.h's.
 *
 * EVERY READ OF THE TEXT AND OF THE READ BUFFER is an aligned dword that holds at least one byte of the interval the slot (or
 * the window) owns: stageBytes (awfm_band_kernel.h) and textDwordAt are the only two places that form such an address.  The
 * text's allocation ends on a 16-byte boundary beyond its last byte and begins on one, so such a dword lies inside it; a dword
 * of the read buffer that holds a byte of the buffer lies in that byte's page.
 *
 * verifyChainsKernel<G>: a wave takes a read (persistent grid over reads), its 64 / G groups of G lanes take the read's slots in
 * turn, lane k of a group is diagonal lo + k of the band.  Unused, malformed, too wide and too long slots are classified from
 * the slot arrays and two reads of the record ends (classifySlot) and cost no row.  The rows of a slot go in chunks of kVerifyChunk: the
 * group stages the chunk's read characters and the text characters its band can touch (at most 64 + 63) into its own words of
 * LDS with aligned dword loads, then runs the rows from LDS bytes -- per row a lane forms t = min(prev[k] + sub, prev[k + 1] + 1)
 * and the horizontal dependency H[k] = min over k' <= k of t[k'] + (k - k') is a min-prefix-scan of t[k'] - k' over the group:
 * log2 G cross-lane steps, no loop over cells.  Cells outside the matrix or the band carry kVerifyInf.  A group's lanes live in
 * one wave and share its control flow, so staging and rows need no workgroup barrier; groups of a wave diverge on their slots'
 * lengths and meet again for the read's best slot.  Vector loads and stores only.
 */
#ifndef AWFM_VERIFY_KERNEL_H
#define AWFM_VERIFY_KERNEL_H

#include "awfm_band_kernel.h"

namespace {

constexpr unsigned kVerifyThreads = 256;    /* per workgroup: four waves, each with reads of its own */
constexpr unsigned kVerifyLdsBytes = 3360;  /* static LDS at G = 16, the most groups: 16 x 52 words and the amino letter table */
constexpr unsigned kVerifyBlocksPerCU = 6;  /* up to 80 VGPRs: six waves per SIMD, i.e. six workgroups of four waves per CU */
static_assert(kVerifyLdsBytes == (kVerifyThreads / 16u) * kVerifyGroupWords * 4u + 32u, "the staging words of sixteen groups and the letter table");
constexpr unsigned kWindowThreads = 256;

struct DevVerifyParams {
  struct AwFmVerifyInputs in;
  struct AwFmVerifyOutputs out;
  const unsigned char *text;
  unsigned long long length;
  const unsigned long long *ends; /* the image's record table; numRecords == 0: one sequence [0, length) */
  unsigned numRecords;
  unsigned long long numReads;
  unsigned slots, pad, drift, amino;
};

/* the aligned dword of the text that begins at position `at` (a multiple of 4, possibly negative or beyond the text), or 0 when
 * it holds no byte of [0, length) */
__device__ __forceinline__ unsigned textDwordAt(const unsigned char *__restrict__ text, unsigned long long length, long long at) {
  return at >= 0 && (unsigned long long)at < length ? *(const unsigned *)(text + at) : 0u;
}

/* Batched recall: the output is one stream of n * width bytes; a thread writes one aligned dword of it (the first thread the
 * bytes ahead of the first aligned dword, the last one a partial tail, bytewise).  The four bytes come from the two aligned
 * dwords of the text that hold them when they belong to one window, and byte by byte where two windows meet. */
__global__ void __launch_bounds__(kWindowThreads)
textWindowsKernel(const unsigned char *__restrict__ text, const unsigned long long length, const unsigned long long *__restrict__ positions,
                  const unsigned long long capacity, const unsigned long long *__restrict__ numOnDevice, const unsigned before,
                  const unsigned width, unsigned char *__restrict__ out) {
  unsigned long long n = capacity;
  if (numOnDevice) {
    const unsigned long long have = *numOnDevice;
    n = have < n ? have : n;
  }
  const unsigned long long total = n * width;
  const unsigned head = (unsigned)((4u - ((unsigned long long)out & 3u)) & 3u);
  const unsigned long long pieces = total <= head ? 1ull : 1ull + (total - head + 3ull) / 4ull;
  for (unsigned long long t = (unsigned long long)blockIdx.x * kWindowThreads + threadIdx.x; t < pieces;
       t += (unsigned long long)gridDim.x * kWindowThreads) {
    const unsigned long long b0 = t == 0 ? 0ull : head + 4ull * (t - 1ull);
    unsigned long long b1 = t == 0 ? head : b0 + 4ull;
    b1 = b1 < total ? b1 : total;
    if (b1 <= b0) continue;
    const unsigned count = (unsigned)(b1 - b0);
    unsigned long long window = b0 / width;
    unsigned offset = (unsigned)(b0 - window * width);
    unsigned value = 0;
    if (offset + count <= width) { /* one window: the bytes [q, q + count) of the text, zero outside it */
      const unsigned long long p = positions[window];
      if (p < length) {
        const long long q = (long long)p - (long long)before + (long long)offset, first = q & ~3ll;
        const unsigned long long both = ((unsigned long long)textDwordAt(text, length, first + 4) << 32) | textDwordAt(text, length, first);
        value = (unsigned)(both >> (8u * (unsigned)(q & 3ll)));
#pragma unroll
        for (unsigned k = 0; k < 4u; k++) {
          const long long at = q + (long long)k;
          if (at < 0 || (unsigned long long)at >= length) value &= ~(0xFFu << (8u * k));
        }
      }
    } else {
      for (unsigned k = 0; k < count; k++) {
        const unsigned long long p = positions[window];
        const long long at = (long long)p - (long long)before + (long long)offset;
        if (p < length && at >= 0 && (unsigned long long)at < length)
          value |= ((textDwordAt(text, length, at & ~3ll) >> (8u * (unsigned)(at & 3ll))) & 0xFFu) << (8u * k);
        if (++offset == width) {
          offset = 0;
          window++;
        }
      }
    }
    if (count == 4u) {
      *(unsigned *)(out + b0) = value;
    } else {
      for (unsigned k = 0; k < count; k++) out[b0 + k] = (unsigned char)(value >> (8u * k));
    }
  }
}

/* the value of slot `at` of read r (header: UNUSED .. TOO LONG, else H(n, m)); every lane of the group returns it */
template <int G>
__device__ __forceinline__ unsigned verifySlot(const DevVerifyParams &p, const unsigned long long at, const unsigned long long readBegin,
                                               const unsigned long long readLength, const bool readOk, unsigned *sRead, unsigned *sText,
                                               const unsigned char *sAmino, const unsigned k) {
  SlotBand b;
  const unsigned status = classifySlot(p, at, p.in.sequences[at], readLength, readOk, b);
  if (status != kSlotHasBand) return status;
  /* the span alone, and the band relative to it: diagonal 0 is the span's first cell, the drift its last one's */
  const long long n64 = (long long)(b.re - b.rb);
  if (n64 > (long long)AWFM_VERIFY_MAX_LENGTH) return AWFM_VERIFY_TOO_LONG;
  const int n = (int)n64, delta = (int)(b.eD - b.bD), m = n + delta; /* n <= 2^20, |delta| <= 63 */
  const int lo = (delta < 0 ? delta : 0) - (int)p.pad, hi = (delta > 0 ? delta : 0) + (int)p.pad;
  const int d = lo + (int)k;
  const bool inBand = d <= hi;
  const unsigned char *R = p.in.readChars + readBegin + b.rb, *T = p.text + b.S + (unsigned long long)b.tb;
  const unsigned char *sReadBytes = (const unsigned char *)sRead, *sTextBytes = (const unsigned char *)sText;
  int prev = inBand && d >= 0 && d <= m ? d : kVerifyInf; /* row 0: H(0, j) = j */
  for (int i0 = 0; i0 < n; i0 += (int)kVerifyChunk) {
    const int rows = n - i0 < (int)kVerifyChunk ? n - i0 : (int)kVerifyChunk;
    /* the text characters T[j - 1] of the chunk's rows i0 + 1 .. i0 + rows: j - 1 = i - 1 + lo .. i - 1 + hi, cut to [0, m) */
    const int tFrom = i0 + lo > 0 ? i0 + lo : 0, tTo = i0 + rows + hi < m ? i0 + rows + hi : m;
    __builtin_amdgcn_wave_barrier(); /* (the rows of the chunk before have read their bytes) */
    const unsigned rOff = stageBytes<G>(R, (unsigned long long)i0, (unsigned long long)(i0 + rows), sRead, k);
    const unsigned tOff = tTo > tFrom ? stageBytes<G>(T, (unsigned long long)tFrom, (unsigned long long)tTo, sText, k) : 0u;
    __builtin_amdgcn_wave_barrier();
    for (int q = 0; q < rows; q++) {
      const int j = i0 + q + 1 + d;
      const bool inMatrix = inBand && j >= 0 && j <= m;
      const unsigned rLetter = verifyLetter(sAmino, p.amino, sReadBytes[rOff + (unsigned)q]);
      unsigned tLetter = 0xFFu;
      if (inMatrix && j >= 1) tLetter = verifyLetter(sAmino, p.amino, sTextBytes[tOff + (unsigned)(j - 1 - tFrom)]);
      const int sub = rLetter == tLetter && rLetter < (p.amino ? 20u : 4u) ? 0 : 1;
      int up = __shfl_down(prev, 1, G);
      up = k == (unsigned)(G - 1) ? kVerifyInf : up;
      int t = prev + sub < up + 1 ? prev + sub : up + 1;
      t = inMatrix ? t : kVerifyInf;
      int v = t - (int)k; /* H[k] - k = min over k' <= k of t[k'] - k' */
#pragma unroll
      for (int step = 1; step < G; step <<= 1) {
        const int other = __shfl_up(v, step, G);
        v = (int)k >= step && other < v ? other : v;
      }
      prev = inMatrix ? v + (int)k : kVerifyInf;
    }
  }
  return (unsigned)__shfl(prev, delta - lo, G);
}

template <int G>
__global__ void __launch_bounds__(kVerifyThreads) verifyChainsKernel(const DevVerifyParams args) {
  constexpr unsigned kGroupsPerWave = 64u / (unsigned)G;
  /* the slot arrays' addresses live in vector registers: thirteen addresses and the nested loops' masks are more scalar
   * registers than a wave has, and the compiler would spill some of them into lanes of a vector register */
  DevVerifyParams p = args;
  asm volatile("" : "+v"(p.in.sequences), "+v"(p.in.chainAnchors), "+v"(p.in.chainReadBegins), "+v"(p.in.chainReadEnds));
  asm volatile("" : "+v"(p.in.chainBeginDiagonals), "+v"(p.in.chainEndDiagonals), "+v"(p.out.editDistances), "+v"(p.out.bestSlots));
  __shared__ unsigned sStage[kVerifyThreads / (unsigned)G][kVerifyGroupWords];
  __shared__ unsigned char sAmino[32];
  if (threadIdx.x < 32u) sAmino[threadIdx.x] = kAminoTables.letterOfAscii[threadIdx.x];
  __syncthreads();
  const unsigned lane = threadIdx.x & 63u, k = lane % (unsigned)G, groupInWave = lane / (unsigned)G;
  unsigned *sRead = sStage[threadIdx.x / (unsigned)G], *sText = sRead + kVerifyReadWords;
  const unsigned long long numWaves = (unsigned long long)gridDim.x * (kVerifyThreads / 64u);
  unsigned unverified = 0;
  for (unsigned long long r = (unsigned long long)blockIdx.x * (kVerifyThreads / 64u) + threadIdx.x / 64u; r < p.numReads; r += numWaves) {
    const unsigned long long readBegin = p.in.readOffsets[r], readEnd = p.in.readOffsets[r + 1ull];
    const bool readOk = readBegin <= readEnd && readEnd <= p.in.numReadChars;
    unsigned bestDistance = 0xFFFFFFFFu, bestSlot = AWFM_CHAINS_NO_SLOT;
    for (unsigned j = groupInWave; j < p.slots; j += kGroupsPerWave) {
      const unsigned long long at = r * p.slots + j;
      const unsigned distance = verifySlot<G>(p, at, readBegin, readEnd - readBegin, readOk, sRead, sText, sAmino, k);
      if (p.out.editDistances && k == 0u) p.out.editDistances[at] = distance;
      if (distance >= AWFM_VERIFY_TOO_LONG) {
        unverified += distance != AWFM_VERIFY_NONE && k == 0u ? 1u : 0u;
      } else if (distance < bestDistance) { /* (a group meets its slots in ascending order: ties stay with the lowest) */
        bestDistance = distance;
        bestSlot = j;
      }
    }
    /* the smallest (distance, slot) of the wave's groups; a group without a distance holds the largest pair there is */
#pragma unroll
    for (unsigned step = (unsigned)G; step < 64u; step <<= 1) {
      const unsigned otherDistance = (unsigned)__shfl_xor((int)bestDistance, (int)step, 64);
      const unsigned otherSlot = (unsigned)__shfl_xor((int)bestSlot, (int)step, 64);
      const bool take = otherDistance < bestDistance || (otherDistance == bestDistance && otherSlot < bestSlot);
      bestDistance = take ? otherDistance : bestDistance;
      bestSlot = take ? otherSlot : bestSlot;
    }
    if (p.out.bestSlots && lane == 0u) p.out.bestSlots[r] = bestSlot;
  }
  if (p.out.numUnverified) { /* one atomic per wave that met any */
#pragma unroll
    for (int offset = 32; offset > 0; offset >>= 1) unverified += (unsigned)__shfl_xor((int)unverified, offset, 64);
    if (lane == 0u && unverified) atomicAdd((unsigned long long *)p.out.numUnverified, (unsigned long long)unverified);
  }
}

}  // namespace

#endif
