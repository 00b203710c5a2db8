/*
 * awfm_insert_kernel.h -- insertHistogramKernel<LDS> and insertIntervalKernel, the kernels of "insert size" (include/awfm_gpu.h).
 * The definition is the header's; the host twins and checkers are awfm_insert.c.
 *
 * HISTOGRAM.  A THREAD takes a pair (persistent grid over pairs, a wave 64 consecutive pairs a trip): the work of a pair is a
 * sequential maximum over 2 C scores with the tie rule "the lowest slot" -- a loop, no cross-lane traffic -- and then ONE load
 * each of sequence, read end and text end per mate, of the best slot only; the score rows of a wave's 64 pairs are one
 * contiguous piece of memory (64 * 2 C words), so every line the wave fetches is used whole.  More lanes a pair would buy
 * coalesced score loads at the price of a keyed maximum across lanes per mate and idle lanes at C that is no power of two.
 * Where do the counts go?  The samples of a real library fall into a few hundred adjacent bins, so one global atomic per pair
 * would queue on a handful of lines at the memory side.  Two tiers:
 *   LDS     (bins <= kInsertLdsBins)  the workgroup zeroes a private histogram of 32-bit counters in static LDS (a workgroup sees
 *           fewer than 2^31 pairs), adds with LDS atomics, and at its end adds only its NONZERO bins to the caller's with 64-bit
 *           global atomics: consecutive lanes, consecutive bins.
 *   global  (above, or $AWFM_GPU_DIAG insert_tier=global) 64-bit global atomics, aggregated over the wave: the lanes that hold
 *           one bin are told by ballots and their first lane adds their number -- one atomic per wave and distinct bin.
 * The two counters are summed over the wave by a butterfly and take one atomic per wave that met any.  The grid gives a workgroup
 * at least kInsertPairsPerBlock pairs (awfm_gpu_insert.hip), so that a small batch does not zero and flush hundreds of private
 * histograms that stay almost empty, and so that few workgroups queue on the same bins of the caller's histogram.
 *
 * INTERVAL.  One workgroup of kIntervalThreads threads.  Each thread sums a contiguous chunk of ceil(bins / threads) bins; one
 * block scan of the sums (a shuffle scan per wave, the waves' totals through LDS) gives every thread the samples before its
 * chunk and every thread N.  The thread whose chunk holds rank_k walks it once more and leaves q_k in LDS; a second pass over
 * the chunks sums i h[i] and h[i] over the inlier bins, one block reduction; thread 0 divides and writes the 64 bytes with
 * ordinary stores.  64-bit integers throughout, no floating point.
 */
#ifndef AWFM_INSERT_KERNEL_H
#define AWFM_INSERT_KERNEL_H

#include "awfm_device.h"

namespace {

constexpr unsigned kInsertThreads = 256;        /* per workgroup: four waves */
constexpr unsigned kInsertLdsBins = 8192;       /* bins of a workgroup's private histogram: 32 KB of 32-bit counters */
constexpr unsigned kInsertLdsBytes = 32768;     /* kInsertLdsBins * 4 */
constexpr unsigned kInsertBlocksPerCU = 4;      /* 4 * 32 KB of the CU's 160 KB of LDS; up to 64 VGPRs: 16 of the 32 waves a CU holds */
constexpr unsigned kInsertMaxVgprs = 64;
constexpr unsigned kInsertPairsPerBlock = 4096; /* a workgroup's least share of the batch: sixteen trips */
constexpr unsigned kIntervalThreads = 1024;     /* the one workgroup of the interval: sixteen waves, at most 64 bins a thread */
constexpr unsigned kIntervalMaxVgprs = 64;
constexpr unsigned kIntervalLdsBytes = 400;     /* 16 waves * (one scan total + two reduction totals) * 8, and four words for three quartiles */

static_assert(kInsertLdsBytes == kInsertLdsBins * 4u, "32-bit counters");

struct DevInsertParams {
  struct AwFmPairInputs in;
  unsigned long long *histogram, *numSamples, *numOutside;
  unsigned long long numPairs;
  long long low, high;
  unsigned slots, floor, minQuality, bins; /* floor: max(minScore, 1) */
};

struct DevIntervalParams {
  const unsigned long long *histogram;
  struct AwFmInsertEstimate *estimate;
  long long low, fallbackMin, fallbackMax;
  unsigned bins, spread, minSamples;
};

/* the best slot of read r, pairing's rules 1 and 2: the largest score that counts, ties to the lowest slot; C: none */
__device__ __forceinline__ unsigned insertBestSlot(const unsigned *scores, const unsigned long long r, const unsigned C, const unsigned floor,
                                                   const bool wellFormed) {
  unsigned best = C, bestScore = 0;
  for (unsigned j = 0; j < C; j++) {
    const unsigned score = scores[r * C + j];
    const bool counts = wellFormed && score < AWFM_VERIFY_TOO_LONG && score >= floor;
    if (counts && (best == C || score > bestScore)) {
      best = j;
      bestScore = score;
    }
  }
  return best;
}

template <bool LDS>
__global__ void __launch_bounds__(kInsertThreads) insertHistogramKernel(const DevInsertParams p) {
  __shared__ unsigned mine[LDS ? kInsertLdsBins : 1];
  const unsigned lane = threadIdx.x & 63u;
  if (LDS) {
    for (unsigned i = threadIdx.x; i < p.bins; i += kInsertThreads) mine[i] = 0u;
    __syncthreads();
  }
  const unsigned C = p.slots;
  const unsigned long long stride = (unsigned long long)gridDim.x * kInsertThreads;
  /* every lane of a wave makes the same number of trips: the ballots want the whole wave */
  unsigned samples = 0, outside = 0;
  for (unsigned long long first = (unsigned long long)blockIdx.x * kInsertThreads + (threadIdx.x & ~63u); first < p.numPairs; first += stride) {
    const unsigned long long pair = first + lane;
    bool isSample = false;
    unsigned bin = 0;
    if (pair < p.numPairs) {
      const unsigned long long A = 2ull * pair, B = A + 1ull;
      const unsigned long long o0 = p.in.readOffsets[A], o1 = p.in.readOffsets[B], o2 = p.in.readOffsets[B + 1ull];
      const unsigned bestA = insertBestSlot(p.in.slotScores, A, C, p.floor, o0 <= o1);
      const unsigned bestB = insertBestSlot(p.in.slotScores, B, C, p.floor, o1 <= o2);
      if (bestA < C && bestB < C) {
        const unsigned long long atA = A * C + bestA, atB = B * C + bestB;
        const unsigned givenA = p.in.mappingQualities ? p.in.mappingQualities[A] : 0u, givenB = p.in.mappingQualities ? p.in.mappingQualities[B] : 0u;
        if (p.in.sequences[atA] == p.in.sequences[atB] && givenA >= p.minQuality && givenB >= p.minQuality) {
          const unsigned long long startA = p.in.slotTextEnds[atA] - p.in.slotReadEnds[atA], startB = p.in.slotTextEnds[atB] - p.in.slotReadEnds[atB];
          const long long T = (long long)(startB + (o2 - o1) - startA);
          isSample = p.low <= T && T <= p.high;
          bin = isSample ? (unsigned)((unsigned long long)T - (unsigned long long)p.low) : 0u; /* < bins <= 65536 */
          samples += isSample ? 1u : 0u;
          outside += isSample ? 0u : 1u;
        }
      }
    }
    if (LDS) {
      if (isSample) atomicAdd(&mine[bin], 1u);
    } else {
      /* the lanes of one bin, found group by group: the first lane of each adds the group's size */
      unsigned long long todo = __builtin_amdgcn_ballot_w64(isSample);
      while (todo != 0ull) {
        const int leader = __builtin_ctzll(todo);
        const unsigned leaderBin = (unsigned)__shfl((int)bin, leader, 64);
        const unsigned long long same = __builtin_amdgcn_ballot_w64(isSample && bin == leaderBin);
        if ((int)lane == leader) atomicAdd(&p.histogram[leaderBin], (unsigned long long)__builtin_popcountll(same));
        todo &= ~same;
      }
    }
  }
  if (LDS) {
    __syncthreads();
    for (unsigned i = threadIdx.x; i < p.bins; i += kInsertThreads) {
      const unsigned count = mine[i];
      if (count) atomicAdd(&p.histogram[i], (unsigned long long)count);
    }
  }
  /* one atomic per wave and counter that met any */
#pragma unroll
  for (int offset = 32; offset > 0; offset >>= 1) {
    samples += (unsigned)__shfl_xor((int)samples, offset, 64);
    outside += (unsigned)__shfl_xor((int)outside, offset, 64);
  }
  if (lane == 0u && samples && p.numSamples) atomicAdd(p.numSamples, (unsigned long long)samples);
  if (lane == 0u && outside && p.numOutside) atomicAdd(p.numOutside, (unsigned long long)outside);
}

__device__ __forceinline__ unsigned long long insertShuffleUp(const unsigned long long x, const int delta) {
  const unsigned low = (unsigned)__shfl_up((int)(unsigned)x, delta, 64), high = (unsigned)__shfl_up((int)(unsigned)(x >> 32), delta, 64);
  return ((unsigned long long)high << 32) | low;
}

__device__ __forceinline__ unsigned long long insertWaveSum(unsigned long long x) {
#pragma unroll
  for (int offset = 32; offset > 0; offset >>= 1) {
    const unsigned low = (unsigned)__shfl_xor((int)(unsigned)x, offset, 64), high = (unsigned)__shfl_xor((int)(unsigned)(x >> 32), offset, 64);
    x += ((unsigned long long)high << 32) | low;
  }
  return x;
}

__device__ __forceinline__ long long insertClamped(const long long x) {
  return x < -AWFM_PAIR_MAX_INSERT ? -AWFM_PAIR_MAX_INSERT : x > AWFM_PAIR_MAX_INSERT ? AWFM_PAIR_MAX_INSERT : x;
}

__global__ void __launch_bounds__(kIntervalThreads) insertIntervalKernel(const DevIntervalParams p) {
  constexpr unsigned kWaves = kIntervalThreads / 64u;
  __shared__ unsigned long long waveTotals[kWaves], weightedTotals[kWaves], inlierTotals[kWaves];
  __shared__ unsigned quartileBins[4]; /* (three, and padding) */
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x / 64u;
  const unsigned chunk = (p.bins + kIntervalThreads - 1u) / kIntervalThreads;
  const unsigned begin = threadIdx.x * chunk < p.bins ? threadIdx.x * chunk : p.bins;
  const unsigned end = begin + chunk < p.bins ? begin + chunk : p.bins;
  unsigned long long sum = 0;
  for (unsigned i = begin; i < end; i++) sum += p.histogram[i];
  /* the samples before this thread's chunk, and N */
  unsigned long long inclusive = sum;
#pragma unroll
  for (int delta = 1; delta < 64; delta <<= 1) {
    const unsigned long long other = insertShuffleUp(inclusive, delta);
    inclusive += (int)lane >= delta ? other : 0ull;
  }
  if (lane == 63u) waveTotals[wave] = inclusive;
  __syncthreads();
  unsigned long long before = inclusive - sum, N = 0;
  for (unsigned w = 0; w < kWaves; w++) {
    before += w < wave ? waveTotals[w] : 0ull;
    N += waveTotals[w];
  }
  struct AwFmInsertEstimate *out = p.estimate;
  if (N < (p.minSamples > 1u ? p.minSamples : 1u)) { /* (the same in every thread) */
    if (threadIdx.x == 0u) {
      out->minInsert = p.fallbackMin;
      out->maxInsert = p.fallbackMax;
      out->quartiles[0] = out->quartiles[1] = out->quartiles[2] = 0;
      out->mean = 0;
      out->numSamples = N;
      out->valid = 0;
    }
    return;
  }
  /* rank_k lies in exactly one chunk: the one with before < rank_k <= before + sum */
#pragma unroll
  for (unsigned k = 1; k <= 3u; k++) {
    const unsigned long long rank = ((unsigned long long)k * N + 3ull) / 4ull;
    if (before < rank && rank <= before + sum) {
      unsigned long long running = before;
      unsigned i = begin;
      for (; i < end; i++) {
        running += p.histogram[i];
        if (running >= rank) break;
      }
      quartileBins[k - 1u] = i;
    }
  }
  __syncthreads();
  const long long q1 = p.low + (long long)quartileBins[0], q2 = p.low + (long long)quartileBins[1], q3 = p.low + (long long)quartileBins[2];
  const long long range = q3 - q1, w = (long long)p.spread * (range > 1 ? range : 1);
  const long long minInsert = insertClamped(q1 - w), maxInsert = insertClamped(q3 + w);
  /* the mean over the inlier bins */
  unsigned long long weighted = 0, inliers = 0;
  for (unsigned i = begin; i < end; i++) {
    const long long T = p.low + (long long)i;
    if (T < minInsert || T > maxInsert) continue;
    const unsigned long long count = p.histogram[i];
    weighted += (unsigned long long)i * count;
    inliers += count;
  }
  weighted = insertWaveSum(weighted);
  inliers = insertWaveSum(inliers);
  if (lane == 0u) {
    weightedTotals[wave] = weighted;
    inlierTotals[wave] = inliers;
  }
  __syncthreads();
  if (threadIdx.x == 0u) {
    weighted = inliers = 0;
    for (unsigned w2 = 0; w2 < kWaves; w2++) {
      weighted += weightedTotals[w2];
      inliers += inlierTotals[w2];
    }
    out->minInsert = minInsert;
    out->maxInsert = maxInsert;
    out->quartiles[0] = q1;
    out->quartiles[1] = q2;
    out->quartiles[2] = q3;
    out->mean = p.low + (long long)(weighted / inliers);
    out->numSamples = N;
    out->valid = 1;
  }
}

}  // namespace

#endif
