/*
 * awfm_align_kernel.h -- alignChainsKernel<G>, the kernel of "chain alignment" (include/awfm_gpu.h): the banded fitting alignment
 * of every read against the record its chosen slot names, with the walk back that emits the edit script.  The definition is
 * the header's; the host twin and checker is awfm_align.c.
 *
 * A group of G lanes per read (persistent grid over reads), lane k is diagonal lo + k of the band in sequence-local coordinates,
 * the rows go in chunks of kVerifyChunk.  The classification of the slot, the band and the staging of a chunk's read characters
 * and text characters (at most 64 + 63, cut to [0, L) of the record) into the group's words of LDS are awfm_band_kernel.h's
 * (classifySlot, readBand, stageChunk) -- EVERY LOAD OF TEXT OR READ is an aligned dword that holds a byte the slot owns, and
 * the record is checked against the text's length before anything is read; only aligned reads load text.  Per row a
 * lane forms the diagonal and the upper candidate, the horizontal dependency is the min-prefix-scan, and the lane derives the
 * cell's 2-bit code from the three candidates: 0 diagonal with equal letters, 1 diagonal with a substitution, 2 up, 3 left.
 *
 * THE TRACE.  Two wave-wide ballots give the codes of a row; a group keeps its 2 G bits of them, G / 4 bytes, and lane 0 stores
 * them as row i - 1 of the group's part of the wave's arena in dScratch: 16 bytes per row and wave whatever G, maxRows rows per
 * wave of the grid.  After the last row a fence orders the stores before the loads of the walk: every lane of the group walks
 * back from the end cell (the smallest (H, t) of row n, a butterfly over the group) through the arena -- the same addresses in
 * all of them, the same state --, lane 0 writes the runs, last to first, and turns them round when they fit maxOps.  Counters
 * take one atomic per wave.  Vector loads and stores only.
 */
#ifndef AWFM_ALIGN_KERNEL_H
#define AWFM_ALIGN_KERNEL_H

#include "awfm_band_kernel.h"

namespace {

constexpr unsigned kAlignThreads = 256;    /* per workgroup: four waves */
constexpr unsigned kAlignLdsBytes = 3360;  /* static LDS at G = 16, the most groups: 16 x 52 words and the amino letter table */
constexpr unsigned kAlignBlocksPerCU = 4;  /* up to 128 VGPRs: four waves per SIMD, i.e. four workgroups of four waves per CU */
constexpr unsigned kAlignRowBytes = 16;    /* of trace per row and wave */
static_assert(kAlignLdsBytes == (kAlignThreads / 16u) * kVerifyGroupWords * 4u + 32u, "the staging words of sixteen groups and the letter table");

struct DevAlignParams {
  struct AwFmVerifyInputs in;
  struct AwFmAlignOutputs out;
  const unsigned *chosen;
  const unsigned char *text;
  unsigned long long length;
  const unsigned long long *ends; /* the image's record table; numRecords == 0: one sequence [0, length) */
  unsigned numRecords;
  unsigned long long numReads;
  unsigned char *arena; /* kAlignRowBytes * maxRows bytes per wave of the grid */
  unsigned slots, pad, drift, amino, maxOps, maxRows;
};

struct DevAlignment {
  unsigned distance, numOps;
  unsigned long long textBegin, textEnd;
};

/* a group's row of trace: G bits of each ballot */
template <int G>
__device__ __forceinline__ void storeTraceRow(unsigned char *trace, unsigned row, unsigned long long b0, unsigned long long b1) {
  if (G == 16) {
    ((unsigned *)trace)[row] = ((unsigned)b0 & 0xFFFFu) | ((unsigned)b1 << 16); /* (above bit 15: the groups behind this one) */
  } else if (G == 32) {
    ((uint2 *)trace)[row] = make_uint2((unsigned)b0, (unsigned)b1);
  } else {
    ((uint4 *)trace)[row] = make_uint4((unsigned)b0, (unsigned)(b0 >> 32), (unsigned)b1, (unsigned)(b1 >> 32));
  }
}

/* the code of lane k's cell in that row */
template <int G>
__device__ __forceinline__ unsigned loadTraceCode(const unsigned char *trace, unsigned row, unsigned k) {
  if (G == 16) {
    const unsigned word = ((const unsigned *)trace)[row];
    return ((word >> k) & 1u) | (((word >> (16u + k)) & 1u) << 1);
  } else if (G == 32) {
    const uint2 word = ((const uint2 *)trace)[row];
    return ((word.x >> k) & 1u) | (((word.y >> k) & 1u) << 1);
  } else {
    const uint4 word = ((const uint4 *)trace)[row];
    const unsigned low = k < 32u ? word.x : word.y, high = k < 32u ? word.z : word.w;
    return ((low >> (k & 31u)) & 1u) | (((high >> (k & 31u)) & 1u) << 1);
  }
}

/* the status of read r (header: UNUSED .. OVERHANG) or its alignment; every lane of the group returns the same */
template <int G>
__device__ __forceinline__ unsigned alignRead(const DevAlignParams &p, const unsigned long long r, unsigned *sRead, unsigned *sText,
                                              const unsigned char *sAmino, unsigned char *trace, const unsigned k, const unsigned groupShift,
                                              DevAlignment &a) {
  const unsigned j = p.chosen[r];
  if (j == AWFM_CHAINS_NO_SLOT) return AWFM_VERIFY_NONE;
  if (j >= p.slots) return AWFM_VERIFY_MALFORMED;
  const unsigned long long at = r * p.slots + j;
  const unsigned long long readBegin = p.in.readOffsets[r], readEnd = p.in.readOffsets[r + 1ull], n64 = readEnd - readBegin;
  SlotBand b;
  const unsigned status = classifySlot(p, at, p.in.sequences[at], n64, readBegin <= readEnd && readEnd <= p.in.numReadChars, b);
  if (status != kSlotHasBand) return status;
  if (n64 > (unsigned long long)p.maxRows) return AWFM_VERIFY_TOO_LONG;
  const int n = (int)n64; /* <= 2^16 */
  const ReadBand band = readBand(b, p.pad);
  const long long lo = band.lo;
  if (band.hi < 0 || lo + (long long)n > b.L) return AWFM_ALIGN_OVERHANG;
  /* lo >= -63 here: hi >= 0 and the band holds at most 64 diagonals */
  const int uMin = band.uMin, uMax = band.uMax;
  const bool inBand = (int)k < band.width;
  const unsigned char *R = p.in.readChars + readBegin, *T = p.text + b.S;
  int prev = inBand && (int)k >= uMin && (int)k <= uMax ? 0 : kVerifyInf; /* row 0: H(0, t) = 0 */
  for (int i0 = 0; i0 < n; i0 += (int)kVerifyChunk) {
    const int rows = n - i0 < (int)kVerifyChunk ? n - i0 : (int)kVerifyChunk;
    const StagedChunk chunk = stageChunk<G>(R, T, band, i0, rows, sRead, sText, k);
    for (int q = 0; q < rows; q++) {
      const int u = i0 + q + 1 + (int)k;
      const bool inMatrix = inBand && u >= uMin && u <= uMax;
      const int sub = stagedSub(chunk, band, sRead, sText, sAmino, p.amino, q, u, inMatrix) ? 1 : 0;
      int up = __shfl_down(prev, 1, G);
      up = k == (unsigned)(G - 1) ? kVerifyInf : up;
      const int diagonal = prev + sub;
      int t = diagonal < up + 1 ? diagonal : up + 1;
      t = inMatrix ? t : kVerifyInf;
      int v = t - (int)k; /* H[k] - k = min over k' <= k of t[k'] - k' */
#pragma unroll
      for (int step = 1; step < G; step <<= 1) {
        const int other = __shfl_up(v, step, G);
        v = (int)k >= step && other < v ? other : v;
      }
      const int h = v + (int)k;
      const unsigned code = diagonal == h ? (unsigned)sub : up + 1 == h ? 2u : 3u;
      const unsigned long long b0 = __builtin_amdgcn_ballot_w64((code & 1u) != 0u), b1 = __builtin_amdgcn_ballot_w64((code >> 1) != 0u);
      if (k == 0u) storeTraceRow<G>(trace, (unsigned)(i0 + q), b0 >> groupShift, b1 >> groupShift);
      prev = inMatrix ? h : kVerifyInf;
    }
  }
  /* the end: the smallest (H, t) of row n.  H <= n + 64 < 2^17 */
  const int uLast = n + (int)k;
  unsigned key = inBand && uLast >= uMin && uLast <= uMax ? ((unsigned)prev << 6) | k : 0xFFFFFFFFu;
#pragma unroll
  for (int step = 1; step < G; step <<= 1) {
    const unsigned other = (unsigned)__shfl_xor((int)key, step, G);
    key = other < key ? other : key;
  }
  a.distance = key >> 6;
  unsigned at2 = key & 63u;
  a.textEnd = (unsigned long long)(lo + (long long)n + (long long)at2);
  __threadfence_block(); /* the rows lane 0 stored are read by every lane of the group */
  unsigned numOps = 0, run = 0, op = 0;
  unsigned *ops = p.out.ops ? p.out.ops + r * p.maxOps : nullptr;
  int i = n;
  /* (n steps to row 0 and at most n + 63 to the left; the bound only matters to a trace that is not this call's own) */
  for (int budget = 2 * n + 64; i > 0 && budget > 0; budget--) {
    const unsigned code = loadTraceCode<G>(trace, (unsigned)(i - 1), at2);
    const unsigned now = code == 0u ? 7u : code == 1u ? 8u : code == 2u ? 1u : 2u;
    if (run && now != op) {
      if (ops && k == 0u && numOps < p.maxOps) ops[numOps] = run << 4 | op;
      numOps++;
      run = 0;
    }
    op = now;
    run++;
    i -= code == 3u ? 0 : 1;
    at2 = code == 2u ? at2 + 1u : code == 3u ? at2 - 1u : at2;
  }
  if (run) {
    if (ops && k == 0u && numOps < p.maxOps) ops[numOps] = run << 4 | op;
    numOps++;
  }
  a.textBegin = (unsigned long long)(lo + (long long)at2);
  a.numOps = numOps;
  if (ops && k == 0u && numOps <= p.maxOps) /* (the lane that stored them: its loads follow its stores) */
    for (unsigned q = 0; q < numOps / 2u; q++) {
      const unsigned other = ops[numOps - 1u - q];
      ops[numOps - 1u - q] = ops[q];
      ops[q] = other;
    }
  return a.distance;
}

template <int G>
__global__ void __launch_bounds__(kAlignThreads) alignChainsKernel(const DevAlignParams args) {
  constexpr unsigned kGroupsPerWave = 64u / (unsigned)G;
  /* the arguments live in vector registers, as the slot arrays' addresses do in verifyChainsKernel: twenty addresses, the
   * nested loops' masks and two ballots a row are more scalar registers than a wave has, and the compiler would spill some of
   * them into lanes of a vector register.  128 vector registers are the budget (four waves per SIMD) */
  DevAlignParams p = args;
  asm volatile("" : "+v"(p.in.sequences), "+v"(p.in.chainAnchors), "+v"(p.in.chainReadBegins), "+v"(p.in.chainReadEnds));
  asm volatile("" : "+v"(p.in.chainBeginDiagonals), "+v"(p.in.chainEndDiagonals), "+v"(p.out.editDistances), "+v"(p.out.textBegins));
  asm volatile("" : "+v"(p.out.textEnds), "+v"(p.out.numOps), "+v"(p.out.ops), "+v"(p.chosen));
  asm volatile("" : "+v"(p.in.readOffsets), "+v"(p.in.readChars), "+v"(p.in.numReadChars), "+v"(p.text));
  asm volatile("" : "+v"(p.ends), "+v"(p.length), "+v"(p.out.numUnaligned), "+v"(p.out.numTruncated));
  asm volatile("" : "+v"(p.numReads), "+v"(p.numRecords), "+v"(p.slots), "+v"(p.pad), "+v"(p.drift), "+v"(p.maxOps), "+v"(p.maxRows));
  __shared__ unsigned sStage[kAlignThreads / (unsigned)G][kVerifyGroupWords];
  __shared__ unsigned char sAmino[32];
  if (threadIdx.x < 32u) sAmino[threadIdx.x] = kAminoTables.letterOfAscii[threadIdx.x];
  __syncthreads();
  const unsigned lane = threadIdx.x & 63u, k = lane % (unsigned)G, groupInWave = lane / (unsigned)G;
  unsigned *sRead = sStage[threadIdx.x / (unsigned)G], *sText = sRead + kVerifyReadWords;
  const unsigned long long wave = (unsigned long long)blockIdx.x * (kAlignThreads / 64u) + threadIdx.x / 64u;
  const unsigned long long numGroups = (unsigned long long)gridDim.x * (kAlignThreads / 64u) * kGroupsPerWave;
  /* the wave's arena, and in it the group's rows of G / 4 bytes */
  unsigned char *trace = p.arena + wave * ((unsigned long long)kAlignRowBytes * p.maxRows) +
                         (unsigned long long)groupInWave * ((unsigned long long)(G / 4) * p.maxRows);
  unsigned unaligned = 0, truncated = 0;
  for (unsigned long long r = wave * kGroupsPerWave + groupInWave; r < p.numReads; r += numGroups) {
    DevAlignment a = {0u, 0u, 0ull, 0ull};
    const unsigned value = alignRead<G>(p, r, sRead, sText, sAmino, trace, k, groupInWave * (unsigned)G, a);
    if (value >= AWFM_ALIGN_OVERHANG) {
      a.numOps = 0u;
      a.textBegin = a.textEnd = 0ull;
      unaligned += value != AWFM_VERIFY_NONE && k == 0u ? 1u : 0u;
    } else {
      truncated += a.numOps > p.maxOps && k == 0u ? 1u : 0u;
    }
    if (k == 0u) {
      if (p.out.editDistances) p.out.editDistances[r] = value;
      if (p.out.textBegins) p.out.textBegins[r] = a.textBegin;
      if (p.out.textEnds) p.out.textEnds[r] = a.textEnd;
      if (p.out.numOps) p.out.numOps[r] = a.numOps;
    }
  }
  /* one atomic per wave and counter that met any */
#pragma unroll
  for (int offset = 32; offset > 0; offset >>= 1) {
    unaligned += (unsigned)__shfl_xor((int)unaligned, offset, 64);
    truncated += (unsigned)__shfl_xor((int)truncated, offset, 64);
  }
  if (lane == 0u && unaligned && p.out.numUnaligned) atomicAdd((unsigned long long *)p.out.numUnaligned, (unsigned long long)unaligned);
  if (lane == 0u && truncated && p.out.numTruncated) atomicAdd((unsigned long long *)p.out.numTruncated, (unsigned long long)truncated);
}

}  // namespace

#endif
