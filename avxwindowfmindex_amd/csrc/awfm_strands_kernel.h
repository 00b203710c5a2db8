/*
 * awfm_strands_kernel.h -- chooseStrandPairsKernel<G>, chooseStrandReadsKernel<G> and orientReadsKernel, the kernels of "strands"
 * (include/awfm_gpu.h).  The definition is the header's; the host twins and checkers are awfm_strands.c.
 *
 * PAIRS.  A group of G lanes takes a pair (persistent grid over pairs, 64 / G pairs a wave in step), as pairMatesKernel does
 * (awfm_pair_mates_kernel.h), with the ORIENTATION as one more coordinate: a concordant candidate has its two strand slots on
 * different strands, so there are two orientations of C x C candidates each -- (m1 on strand 0, m2 on strand 1) and the other
 * way round.  G = 32 (C <= 4): lane k holds orientation k >> 4, slot a = (k >> 2) & 3 of m1 and slot b = k & 3 of m2: one
 * candidate.  G = 64 (C <= 16): lane k holds slot a = k >> 2 of m1 on BOTH strands and the slots b = k % 4 + 4 t, t < 4, of
 * m2 on both: eight candidates.  Each lane loads its strand slots ONCE (once per LANE: at G = 32 a slot of either mate lies in four lanes, at G = 64 a slot
 * of m1 in four and a slot of m2 in sixteen, each with a load of its own) -- score, read end, text end, sequence -- and the
 * pair's six read offsets; everything after that is registers and cross-lane moves: no LDS, no atomics but the counters.
 * Keyed maxima over the group (a butterfly of __shfl_xor each, so every lane ends with the result):
 *   each read's best    (score + 1) << 5 | 31 - u over its counting strand slots: the largest score, ties to the lowest u.
 *   each read's second  score + 1 over the strand slots that are neither the best nor its duplicate; the best's four words come
 *                       to every lane by __shfl from a lane that holds them.
 *   the winner          exists, value, concordant, 31 - u1, 31 - u2 over the lanes' concordant candidates; the discordant
 *                       candidate (best(m1), best(m2)) lies in no lane when the two are on one strand, so every lane makes it
 *                       from the two bests it already holds and joins it to the maximum: the header's tie rule is the comparison.
 *   the pair's second   the same keys with the winner's duplicates masked out (the winner's eight words come by __shfl).
 * T of the winner is recomputed from those words.  Lane 0 of a group stores the pair's outputs and read m1's, lane 1 read m2's.
 * A quality's division is 32-bit whenever every group of the wave has cap * best below 2^32 (a wave-uniform branch; always, for
 * scores the library wrote), else 64-bit.
 *
 * READS (unpaired).  G = 16: lane k holds slot k on both strands; G = 64: lane k < 32 holds strand k >> 4, slot k & 15.  The
 * two per-read maxima above, and lane 0 stores.
 *
 * ORIENT.  A wave per read (persistent grid), a lane per ALIGNED word of the output, as reverseComplementKernel: the four source
 * bytes of a word -- the same ones of the chosen row for the characters, the forward row's mirrored ones for the qualities of
 * a read on strand 1 -- lie in one or two aligned words of the input, each loaded only when it holds a byte of the buffer,
 * funnelled by v_alignbyte; whole words are stored but at a read's two edges.  Lanes 0 .. C - 1 copy the nine columns.
 * Vector loads and stores only.
 */
#ifndef AWFM_STRANDS_KERNEL_H
#define AWFM_STRANDS_KERNEL_H

#include "awfm_device.h"

namespace {

constexpr unsigned kStrandThreads = 256;   /* per workgroup: four waves */
constexpr unsigned kStrandBlocksPerCU = 4; /* up to 128 VGPRs: four waves per SIMD, i.e. four workgroups of four waves per CU */
constexpr unsigned kStrandMaxVgprs = 128;
constexpr unsigned kStrandLdsBytes = 0;    /* no LDS */
/* the wave per pair holds 2 + 8 strand slots and eight candidates a lane: two waves per SIMD */
constexpr unsigned kStrandWaveBlocksPerCU = 2;
constexpr unsigned kStrandWaveMaxVgprs = 256;
constexpr unsigned kOrientThreads = 256;   /* four waves, each with reads of its own */
constexpr unsigned kOrientBlocksPerCU = 8; /* up to 64 VGPRs: eight waves per SIMD */
constexpr unsigned kOrientMaxVgprs = 64;

struct DevStrandParams {
  struct AwFmStrandInputs in;
  struct AwFmStrandOutputs out;
  unsigned long long numReads; /* R: the rows are 2 R */
  long long minInsert, maxInsert, pad;
  unsigned slots, floor, penalty, cap; /* floor: max(minScore, 1) */
};

struct DevOrientParams {
  struct AwFmOrientInputs in;
  struct AwFmOrientOutputs out;
  unsigned long long numReads;
  unsigned slots;
};

/* the launch's parameters where the launch left them, in the kernel's argument segment (pairMatesKernel does the same) */
typedef const __attribute__((address_space(4))) DevStrandParams *StrandParamsRef;

/* a strand slot in registers; score 0: it does not count (a counting score is >= 1) */
struct StrandSlot {
  unsigned score, seq, end, low, high;
};

__device__ __forceinline__ StrandSlot strandSlotNone() { return StrandSlot{0u, 0u, 0u, 0u, 0u}; }

/* slot j of `row` */
__device__ __forceinline__ StrandSlot strandSlotLoad(StrandParamsRef p, const unsigned long long row, const unsigned j, const bool wellFormed) {
  StrandSlot s;
  const unsigned long long at = row * p->slots + j;
  s.score = p->in.slotScores[at];
  s.seq = p->in.sequences[at];
  s.end = p->in.slotReadEnds[at];
  const unsigned long long textEnd = p->in.slotTextEnds[at];
  s.low = (unsigned)textEnd;
  s.high = (unsigned)(textEnd >> 32);
  s.score = wellFormed && s.score < AWFM_VERIFY_TOO_LONG && s.score >= p->floor ? s.score : 0u;
  return s;
}

__device__ __forceinline__ long long strandStart(const StrandSlot &s) {
  return (long long)((((unsigned long long)s.high << 32) | s.low) - (unsigned long long)s.end);
}

/* rule 3 for two counting strand slots on one strand */
__device__ __forceinline__ bool strandSameCell(const StrandSlot &x, const StrandSlot &y) {
  return x.seq == y.seq && x.end == y.end && x.low == y.low && x.high == y.high;
}

template <int G>
__device__ __forceinline__ unsigned long long strandGroupMax(unsigned long long key) {
#pragma unroll
  for (int step = 1; step < G; step <<= 1) {
    const unsigned otherLow = (unsigned)__shfl_xor((int)(unsigned)key, step, G), otherHigh = (unsigned)__shfl_xor((int)(unsigned)(key >> 32), step, G);
    const unsigned long long other = ((unsigned long long)otherHigh << 32) | otherLow;
    key = other > key ? other : key;
  }
  return key;
}

template <int G>
__device__ __forceinline__ unsigned strandGroupMax32(unsigned key) {
#pragma unroll
  for (int step = 1; step < G; step <<= 1) {
    const unsigned other = (unsigned)__shfl_xor((int)key, step, G);
    key = other > key ? other : key;
  }
  return key;
}

/* the four words of a strand slot's end cell from lane `holder` of the group, which holds it in `mine` */
template <int G>
__device__ __forceinline__ StrandSlot strandFetch(const StrandSlot &mine, const int holder) {
  StrandSlot s;
  s.score = 1u;
  s.seq = (unsigned)__shfl((int)mine.seq, holder, G);
  s.end = (unsigned)__shfl((int)mine.end, holder, G);
  s.low = (unsigned)__shfl((int)mine.low, holder, G);
  s.high = (unsigned)__shfl((int)mine.high, holder, G);
  return s;
}

/* rule 5 and pair mates' rule 6: floor(cap * (best - second) / best), 0 when `has` is false; best < 2^33 */
__device__ __forceinline__ unsigned strandQuality(const unsigned cap, const unsigned long long best, const unsigned long long second, const bool has) {
  const unsigned long long numerator = has ? (unsigned long long)cap * (best - second) : 0ull, denominator = has ? best : 1ull;
  if (__builtin_amdgcn_ballot_w64((numerator | denominator) >> 32 != 0ull) == 0ull) return (unsigned)numerator / (unsigned)denominator;
  return (unsigned)(numerator / denominator);
}

/* strand and slot of strand slot u */
__device__ __forceinline__ unsigned strandOf(const unsigned u, const unsigned C) { return u >= C ? 1u : 0u; }
__device__ __forceinline__ unsigned slotOf(const unsigned u, const unsigned C) { return u >= C ? u - C : u; }

/* T of rule 6 for x of m1 on strand `sigma1` and y of m2 on the other strand */
__device__ __forceinline__ long long strandTemplate(const StrandSlot &x, const StrandSlot &y, const unsigned sigma1, const long long n1, const long long n2) {
  const unsigned long long s1 = (unsigned long long)strandStart(x), s2 = (unsigned long long)strandStart(y);
  return sigma1 == 0u ? (long long)(s2 + (unsigned long long)n2 - s1) : (long long)(s1 + (unsigned long long)n1 - s2);
}

/* the per-read and per-row outputs of read r (one lane) */
__device__ __forceinline__ void strandStoreRead(StrandParamsRef p, const unsigned long long r, const bool hasChosen, const unsigned chosen,
                                                const unsigned bestScore, const unsigned secondScore, const unsigned quality,
                                                const int windowStrand, const unsigned windowSequence, const long long windowBegin,
                                                const long long windowEnd) {
  const unsigned C = p->slots;
  const unsigned strand = hasChosen ? strandOf(chosen, C) : 0u, slot = hasChosen ? slotOf(chosen, C) : AWFM_CHAINS_NO_SLOT;
  if (p->out.strands) p->out.strands[r] = (unsigned char)strand;
  if (p->out.strandSlots) p->out.strandSlots[r] = slot;
  if (p->out.bestScores) p->out.bestScores[r] = bestScore;
  if (p->out.secondScores) p->out.secondScores[r] = secondScore;
  if (p->out.mappingQualities) p->out.mappingQualities[r] = (unsigned char)quality;
  if (p->out.baseFlags) p->out.baseFlags[r] = strand ? (unsigned short)0x10 : (unsigned short)0;
#pragma unroll
  for (int sigma = 0; sigma < 2; sigma++) {
    const unsigned long long row = (sigma ? p->numReads : 0ull) + r;
    const bool here = windowStrand == sigma;
    if (p->out.rowSlots) p->out.rowSlots[row] = hasChosen && strand == (unsigned)sigma ? slot : AWFM_CHAINS_NO_SLOT;
    if (p->out.windowSequences) p->out.windowSequences[row] = here ? windowSequence : AWFM_CANDIDATES_NONE;
    if (p->out.windowBegins) p->out.windowBegins[row] = here ? (unsigned long long)windowBegin : 0ull;
    if (p->out.windowEnds) p->out.windowEnds[row] = here ? (unsigned long long)windowEnd : 0ull;
  }
}

constexpr unsigned long long kStrandKeyExists = 1ull << 44; /* value < 2^33 above concordant << 10 | 31 - u1 << 5 | 31 - u2 */

template <int G>
__global__ void __launch_bounds__(kStrandThreads, G == 64 ? 2 : 4) chooseStrandPairsKernel(const DevStrandParams args) {
  (void)args; /* (the struct is the kernel's only argument, so it begins the segment) */
  StrandParamsRef p = (StrandParamsRef)__builtin_amdgcn_kernarg_segment_ptr();
  constexpr int O = G == 64 ? 2 : 1, Q = G == 64 ? 4 : 1;
  constexpr unsigned kGroupsPerBlock = kStrandThreads / (unsigned)G;
  const unsigned lane = threadIdx.x & 63u, k = lane % (unsigned)G;
  const unsigned a = G == 64 ? k >> 2 : (k >> 2) & 3u, column = k & 3u, orientation = G == 64 ? 0u : k >> 4;
  const unsigned long long stride = (unsigned long long)gridDim.x * kGroupsPerBlock;
  /* every group of a wave makes the same number of trips: the cross-lane moves want the whole wave */
  const unsigned long long waveFirst = (unsigned long long)blockIdx.x * kGroupsPerBlock + (threadIdx.x / 64u) * (64u / (unsigned)G);
  unsigned reverse = 0, proper = 0, windows = 0, malformed = 0;
  for (unsigned long long first = waveFirst; first < p->numReads >> 1; first += stride) {
    asm volatile("" : "+s"(p));
    const unsigned C = p->slots;
    const unsigned long long numPairs = p->numReads >> 1;
    const unsigned long long pair = first + lane / (unsigned)G;
    const bool active = pair < numPairs;
    const unsigned long long m1 = 2ull * pair, R = p->numReads;
    unsigned long long f0 = 0, f1 = 0, f2 = 0, v0 = 0, v1 = 0, v2 = 0;
    if (active) {
      f0 = p->in.readOffsets[m1];
      f1 = p->in.readOffsets[m1 + 1ull];
      f2 = p->in.readOffsets[m1 + 2ull];
      v0 = p->in.readOffsets[R + m1];
      v1 = p->in.readOffsets[R + m1 + 1ull];
      v2 = p->in.readOffsets[R + m1 + 2ull];
    }
    const long long n1 = (long long)(f1 - f0), n2 = (long long)(f2 - f1);
    const bool bad1 = f0 > f1 || v0 > v1 || f1 - f0 != v1 - v0, bad2 = f1 > f2 || v1 > v2 || f2 - f1 != v2 - v1;
    /* the lane's strand slots: x[i] of m1 on strand sigma(i), y[i][t] of m2 on the other strand */
    StrandSlot x[O], y[O][Q];
#pragma unroll
    for (int i = 0; i < O; i++) {
      const unsigned sigma = O == 2 ? (unsigned)i : orientation;
      x[i] = strandSlotNone();
      if (active && a < C) x[i] = strandSlotLoad(p, (sigma ? R : 0ull) + m1, a, !bad1);
#pragma unroll
      for (int t = 0; t < Q; t++) {
        const unsigned b = column + 4u * (unsigned)t;
        y[i][t] = strandSlotNone();
        if (active && b < C) y[i][t] = strandSlotLoad(p, (sigma ? 0ull : R) + m1 + 1ull, b, !bad2);
      }
    }
    /* rule 2: each read's best */
    unsigned long long bestKey1 = 0, bestKey2 = 0;
#pragma unroll
    for (int i = 0; i < O; i++) {
      const unsigned sigma = O == 2 ? (unsigned)i : orientation;
      const unsigned long long key1 = (((unsigned long long)x[i].score + 1ull) << 5) | (31u - (sigma * C + a));
      bestKey1 = (x[i].score != 0u) && key1 > bestKey1 ? key1 : bestKey1;
#pragma unroll
      for (int t = 0; t < Q; t++) {
        const unsigned b = column + 4u * (unsigned)t;
        const unsigned long long key2 = (((unsigned long long)y[i][t].score + 1ull) << 5) | (31u - ((1u - sigma) * C + b));
        bestKey2 = (y[i][t].score != 0u) && key2 > bestKey2 ? key2 : bestKey2;
      }
    }
    bestKey1 = strandGroupMax<G>(bestKey1);
    bestKey2 = strandGroupMax<G>(bestKey2);
    const bool has1 = bestKey1 != 0ull, has2 = bestKey2 != 0ull;
    const unsigned best1 = has1 ? 31u - ((unsigned)bestKey1 & 31u) : 0u, best2 = has2 ? 31u - ((unsigned)bestKey2 & 31u) : 0u;
    const unsigned bestScore1 = has1 ? (unsigned)(bestKey1 >> 5) - 1u : 0u, bestScore2 = has2 ? (unsigned)(bestKey2 >> 5) - 1u : 0u;
    /* a strand slot of m1 or of m2, in every lane, from a lane that holds it (uniform over the group) */
    auto fetch1 = [&](const unsigned u) {
      const unsigned sigma = strandOf(u, C), j = slotOf(u, C);
      const StrandSlot mine = O == 2 && sigma ? x[O - 1] : x[0];
      return strandFetch<G>(mine, (int)(O == 2 ? j << 2 : (sigma << 4) | (j << 2)) & (G - 1));
    };
    auto fetch2 = [&](const unsigned u) {
      const unsigned sigma = strandOf(u, C), j = slotOf(u, C);
      StrandSlot mine = y[0][0];
#pragma unroll
      for (int i = 0; i < O; i++)
#pragma unroll
        for (int t = 0; t < Q; t++)
          if ((O == 1 || (unsigned)i == 1u - sigma) && (j >> 2) == (unsigned)t) mine = y[i][t];
      return strandFetch<G>(mine, (int)(O == 2 ? j & 3u : ((1u - sigma) << 4) | (j & 3u)) & (G - 1));
    };
    const StrandSlot top1 = fetch1(best1), top2 = fetch2(best2);
    const unsigned sigmaTop1 = strandOf(best1, C), sigmaTop2 = strandOf(best2, C);
    /* rules 3 and 4: each read's second */
    unsigned secondKey1 = 0, secondKey2 = 0;
#pragma unroll
    for (int i = 0; i < O; i++) {
      const unsigned sigma = O == 2 ? (unsigned)i : orientation;
      const unsigned u1 = sigma * C + a;
      const bool same1 = u1 == best1 || (sigma == sigmaTop1 && strandSameCell(x[i], top1));
      const unsigned key1 = (x[i].score != 0u) && !same1 ? x[i].score + 1u : 0u;
      secondKey1 = key1 > secondKey1 ? key1 : secondKey1;
#pragma unroll
      for (int t = 0; t < Q; t++) {
        const unsigned u2 = (1u - sigma) * C + column + 4u * (unsigned)t;
        const bool same2 = u2 == best2 || (1u - sigma == sigmaTop2 && strandSameCell(y[i][t], top2));
        const unsigned key2 = (y[i][t].score != 0u) && !same2 ? y[i][t].score + 1u : 0u;
        secondKey2 = key2 > secondKey2 ? key2 : secondKey2;
      }
    }
    secondKey1 = strandGroupMax32<G>(secondKey1);
    secondKey2 = strandGroupMax32<G>(secondKey2);
    const unsigned secondScore1 = secondKey1 ? secondKey1 - 1u : 0u, secondScore2 = secondKey2 ? secondKey2 - 1u : 0u;
    const unsigned quality1 = strandQuality(p->cap, bestScore1, secondScore1, has1), quality2 = strandQuality(p->cap, bestScore2, secondScore2, has2);
    /* rule 6: the lane's concordant candidates */
    const long long minInsert = p->minInsert, maxInsert = p->maxInsert;
    auto candidateKey = [&](const StrandSlot &first, const StrandSlot &other, const unsigned sigma, const unsigned u1, const unsigned u2) {
      const long long T = strandTemplate(first, other, sigma, n1, n2);
      const bool concordant = first.score != 0u && other.score != 0u && first.seq == other.seq && minInsert <= T && T <= maxInsert;
      const unsigned long long value = (unsigned long long)first.score + other.score;
      return concordant ? kStrandKeyExists | (value << 11) | 1024ull | ((31u - u1) << 5) | (31u - u2) : 0ull;
    };
    unsigned long long winnerKey = 0;
#pragma unroll
    for (int i = 0; i < O; i++) {
      const unsigned sigma = O == 2 ? (unsigned)i : orientation;
#pragma unroll
      for (int t = 0; t < Q; t++) {
        const unsigned long long key = candidateKey(x[i], y[i][t], sigma, sigma * C + a, (1u - sigma) * C + column + 4u * (unsigned)t);
        winnerKey = key > winnerKey ? key : winnerKey;
      }
    }
    winnerKey = strandGroupMax<G>(winnerKey);
    /* rule 7: the discordant candidate, the same in every lane of the group */
    unsigned long long discordantKey = 0;
    if (has1 && has2) {
      const long long T = strandTemplate(top1, top2, sigmaTop1, n1, n2);
      const bool concordant = sigmaTop1 != sigmaTop2 && top1.seq == top2.seq && minInsert <= T && T <= maxInsert;
      const unsigned long long sum = (unsigned long long)bestScore1 + bestScore2, value = sum > p->penalty ? sum - p->penalty : 0ull;
      if (!concordant) discordantKey = kStrandKeyExists | (value << 11) | ((31u - best1) << 5) | (31u - best2);
    }
    winnerKey = discordantKey > winnerKey ? discordantKey : winnerKey;
    const bool hasWinner = winnerKey != 0ull, isProper = (winnerKey & 1024ull) != 0ull;
    const unsigned chosen1 = hasWinner ? 31u - ((unsigned)(winnerKey >> 5) & 31u) : best1, chosen2 = hasWinner ? 31u - ((unsigned)winnerKey & 31u) : best2;
    const StrandSlot won1 = fetch1(chosen1), won2 = fetch2(chosen2);
    const unsigned sigmaWon1 = strandOf(chosen1, C), sigmaWon2 = strandOf(chosen2, C);
    /* pair mates' rule 5: the second, the winner's duplicates masked out (both of the winner's strand slots count) */
    unsigned long long secondKey = 0;
#pragma unroll
    for (int i = 0; i < O; i++) {
      const unsigned sigma = O == 2 ? (unsigned)i : orientation;
      const bool same1 = sigma * C + a == chosen1 || ((x[i].score != 0u) && sigma == sigmaWon1 && strandSameCell(x[i], won1));
#pragma unroll
      for (int t = 0; t < Q; t++) {
        const unsigned u2 = (1u - sigma) * C + column + 4u * (unsigned)t;
        const bool same2 = u2 == chosen2 || ((y[i][t].score != 0u) && 1u - sigma == sigmaWon2 && strandSameCell(y[i][t], won2));
        const unsigned long long key = same1 && same2 ? 0ull : candidateKey(x[i], y[i][t], sigma, sigma * C + a, u2);
        secondKey = key > secondKey ? key : secondKey;
      }
    }
    secondKey = strandGroupMax<G>(secondKey);
    {
      const bool same1 = best1 == chosen1 || (sigmaTop1 == sigmaWon1 && strandSameCell(top1, won1));
      const bool same2 = best2 == chosen2 || (sigmaTop2 == sigmaWon2 && strandSameCell(top2, won2));
      const unsigned long long key = same1 && same2 ? 0ull : discordantKey;
      secondKey = key > secondKey ? key : secondKey;
    }
    const unsigned long long win = (winnerKey >> 11) & 0x1FFFFFFFFull, second = (secondKey >> 11) & 0x1FFFFFFFFull;
    const unsigned quality = strandQuality(p->cap, win, second, isProper);
    const long long length = strandTemplate(won1, won2, sigmaWon1, n1, n2);
    unsigned long long value = win;
    if (!hasWinner) value = has1 ? bestScore1 : has2 ? bestScore2 : 0u;
    if (active && k == 0u) {
      proper += isProper ? 1u : 0u;
      if (p->out.properPairs) p->out.properPairs[pair] = isProper ? 1 : 0;
      if (p->out.pairScores) p->out.pairScores[pair] = (unsigned)value;
      if (p->out.pairSecondScores) p->out.pairSecondScores[pair] = (unsigned)second;
      if (p->out.templateLengths) p->out.templateLengths[pair] = isProper ? length : 0ll;
      if (p->out.pairQualities) p->out.pairQualities[pair] = (unsigned char)quality;
    }
    if (active && k < 2u) { /* lane 0: read m1, lane 1: read m2 */
      const bool second2 = k == 1u;
      const bool placed = second2 ? has2 : has1, matePlaced = second2 ? has1 : has2;
      const unsigned chosen = second2 ? chosen2 : chosen1, best = second2 ? best2 : best1, given = second2 ? quality2 : quality1;
      const bool hasChosen = hasWinner || placed;
      unsigned mine = given;
      if (isProper) {
        mine = chosen == best ? given : 0u;
        mine = quality > mine ? quality : mine;
      }
      /* rule 10: the window the mate's best strand slot names, on the other strand */
      int windowStrand = -1;
      unsigned windowSequence = AWFM_CANDIDATES_NONE;
      long long windowBegin = 0, windowEnd = 0;
      if (!isProper && matePlaced) {
        const StrandSlot &mate = second2 ? top1 : top2;
        const unsigned long long S = (unsigned long long)strandStart(mate), pad = (unsigned long long)p->pad;
        const unsigned long long nMine = (unsigned long long)(second2 ? n2 : n1), nMate = (unsigned long long)(second2 ? n1 : n2);
        windowSequence = mate.seq;
        if ((second2 ? sigmaTop1 : sigmaTop2) == 0u) {
          windowStrand = 1;
          windowBegin = (long long)(S + (unsigned long long)minInsert - nMine - pad);
          windowEnd = (long long)(S + (unsigned long long)maxInsert + pad);
        } else {
          const unsigned long long E = S + nMate;
          windowStrand = 0;
          windowBegin = (long long)(E - (unsigned long long)maxInsert - pad);
          windowEnd = (long long)(E - (unsigned long long)minInsert + nMine + pad);
        }
        windowBegin = windowBegin < 0 ? 0 : windowBegin;
        windowEnd = windowEnd < 0 ? 0 : windowEnd;
        windows++;
      }
      reverse += hasChosen ? strandOf(chosen, C) : 0u;
      malformed += (second2 ? bad2 : bad1) ? 1u : 0u;
      strandStoreRead(p, m1 + k, hasChosen, chosen, second2 ? bestScore2 : bestScore1, second2 ? secondScore2 : secondScore1, mine, windowStrand,
                      windowSequence, windowBegin, windowEnd);
    }
  }
  /* one atomic per wave and counter that met any */
#pragma unroll
  for (int offset = 32; offset > 0; offset >>= 1) {
    reverse += (unsigned)__shfl_xor((int)reverse, offset, 64);
    proper += (unsigned)__shfl_xor((int)proper, offset, 64);
    windows += (unsigned)__shfl_xor((int)windows, offset, 64);
    malformed += (unsigned)__shfl_xor((int)malformed, offset, 64);
  }
  if (lane == 0u && reverse && p->out.numReverse) atomicAdd((unsigned long long *)p->out.numReverse, (unsigned long long)reverse);
  if (lane == 0u && proper && p->out.numProper) atomicAdd((unsigned long long *)p->out.numProper, (unsigned long long)proper);
  if (lane == 0u && windows && p->out.numWindows) atomicAdd((unsigned long long *)p->out.numWindows, (unsigned long long)windows);
  if (lane == 0u && malformed && p->out.numMalformed) atomicAdd((unsigned long long *)p->out.numMalformed, (unsigned long long)malformed);
}

template <int G>
__global__ void __launch_bounds__(kStrandThreads, 4) chooseStrandReadsKernel(const DevStrandParams args) {
  (void)args;
  StrandParamsRef p = (StrandParamsRef)__builtin_amdgcn_kernarg_segment_ptr();
  constexpr int O = G == 64 ? 1 : 2;
  constexpr unsigned kGroupsPerBlock = kStrandThreads / (unsigned)G;
  const unsigned lane = threadIdx.x & 63u, k = lane % (unsigned)G, j = k & 15u;
  const unsigned C = p->slots;
  const unsigned long long stride = (unsigned long long)gridDim.x * kGroupsPerBlock;
  const unsigned long long waveFirst = (unsigned long long)blockIdx.x * kGroupsPerBlock + (threadIdx.x / 64u) * (64u / (unsigned)G);
  unsigned reverse = 0, malformed = 0;
  for (unsigned long long first = waveFirst; first < p->numReads; first += stride) {
    asm volatile("" : "+s"(p));
    const unsigned long long r = first + lane / (unsigned)G, R = p->numReads;
    const bool active = r < R;
    unsigned long long f0 = 0, f1 = 0, v0 = 0, v1 = 0;
    if (active) {
      f0 = p->in.readOffsets[r];
      f1 = p->in.readOffsets[r + 1ull];
      v0 = p->in.readOffsets[R + r];
      v1 = p->in.readOffsets[R + r + 1ull];
    }
    const bool bad = f0 > f1 || v0 > v1 || f1 - f0 != v1 - v0;
    /* the lane's strand slots: slot j on both strands (G = 16), or on strand k >> 4 for k < 32 (G = 64) */
    StrandSlot x[O];
    unsigned long long bestKey = 0;
#pragma unroll
    for (int i = 0; i < O; i++) {
      const unsigned sigma = O == 2 ? (unsigned)i : k >> 4;
      x[i] = strandSlotNone();
      if (active && j < C && sigma < 2u) x[i] = strandSlotLoad(p, (sigma ? R : 0ull) + r, j, !bad);
      const unsigned long long key = (((unsigned long long)x[i].score + 1ull) << 5) | (31u - ((sigma & 1u) * C + j));
      bestKey = (x[i].score != 0u) && key > bestKey ? key : bestKey;
    }
    bestKey = strandGroupMax<G>(bestKey);
    const bool has = bestKey != 0ull;
    const unsigned best = has ? 31u - ((unsigned)bestKey & 31u) : 0u, bestScore = has ? (unsigned)(bestKey >> 5) - 1u : 0u;
    const unsigned sigmaTop = strandOf(best, C), slotTop = slotOf(best, C);
    const StrandSlot top = strandFetch<G>(O == 2 && sigmaTop ? x[O - 1] : x[0], (int)(O == 2 ? slotTop : (sigmaTop << 4) | slotTop));
    unsigned secondKey = 0;
#pragma unroll
    for (int i = 0; i < O; i++) {
      const unsigned sigma = O == 2 ? (unsigned)i : k >> 4;
      const bool same = sigma * C + j == best || (sigma == sigmaTop && strandSameCell(x[i], top));
      const unsigned key = (x[i].score != 0u) && !same ? x[i].score + 1u : 0u;
      secondKey = key > secondKey ? key : secondKey;
    }
    secondKey = strandGroupMax32<G>(secondKey);
    const unsigned secondScore = secondKey ? secondKey - 1u : 0u;
    const unsigned quality = strandQuality(p->cap, bestScore, secondScore, has);
    if (active && k == 0u) {
      reverse += has ? sigmaTop : 0u;
      malformed += bad ? 1u : 0u;
      strandStoreRead(p, r, has, best, bestScore, secondScore, quality, -1, AWFM_CANDIDATES_NONE, 0, 0);
    }
  }
#pragma unroll
  for (int offset = 32; offset > 0; offset >>= 1) {
    reverse += (unsigned)__shfl_xor((int)reverse, offset, 64);
    malformed += (unsigned)__shfl_xor((int)malformed, offset, 64);
  }
  if (lane == 0u && reverse && p->out.numReverse) atomicAdd((unsigned long long *)p->out.numReverse, (unsigned long long)reverse);
  if (lane == 0u && malformed && p->out.numMalformed) atomicAdd((unsigned long long *)p->out.numMalformed, (unsigned long long)malformed);
}

/* the four bytes [at, at + 4) of the buffer, `at` anywhere from -3 on: from the one or two aligned words that hold them, each
 * loaded only when it holds a byte of the buffer; bytes outside the buffer come as zeros */
__device__ __forceinline__ unsigned orientFour(const unsigned char *chars, const unsigned long long numChars, const long long at) {
  const unsigned shift = (unsigned)((unsigned long long)(uintptr_t)chars + (unsigned long long)at) & 3u;
  const long long first = at - (long long)shift; /* the aligned word that holds byte `at` */
  unsigned low = 0u, high = 0u;
  if (first + 4 > 0 && first < (long long)numChars) low = *(const unsigned *)(chars + first);
  if (shift != 0u && first + 8 > 0 && first + 4 < (long long)numChars) high = *(const unsigned *)(chars + first + 4);
  return __builtin_amdgcn_alignbyte(high, low, shift);
}

/* the n bytes from `from` of the input buffer to `to`, in order or mirrored; a lane per aligned word of the output */
__device__ __forceinline__ void orientCopy(const unsigned char *chars, const unsigned long long numChars, const unsigned long long from,
                                           unsigned char *to, const long long n, const bool mirrored, const unsigned lane) {
  /* the aligned words of the output that hold a byte of the read: the first begins `lead` bytes before the read */
  const long long lead = (long long)((unsigned long long)(uintptr_t)to & 3ull);
  const long long numWords = (n + lead + 3) >> 2;
  for (long long w = lane; w < numWords; w += 64) {
    const long long i = 4 * w - lead; /* the word's first byte as a position of the read: -3 .. n - 1 */
    unsigned word = orientFour(chars, numChars, (long long)from + (mirrored ? n - 4 - i : i));
    if (mirrored) word = __builtin_bswap32(word);
    unsigned char *at = to + i;
    if (i >= 0 && i + 4 <= n) {
      *(unsigned *)at = word;
    } else {
#pragma unroll
      for (int b = 0; b < 4; b++)
        if (i + b >= 0 && i + b < n) at[b] = (unsigned char)(word >> (8 * b));
    }
  }
}

typedef const __attribute__((address_space(4))) DevOrientParams *OrientParamsRef;

__global__ void __launch_bounds__(kOrientThreads, 8) orientReadsKernel(const DevOrientParams args) {
  (void)args; /* (read from the argument segment where a field is used, as above) */
  OrientParamsRef q = (OrientParamsRef)__builtin_amdgcn_kernarg_segment_ptr();
  const unsigned lane = threadIdx.x & 63u;
  const unsigned long long numWaves = (unsigned long long)gridDim.x * (kOrientThreads / 64u), R = q->numReads;
  const unsigned long long *offsets = (const unsigned long long *)q->in.rows.readOffsets;
  const unsigned long long numChars = q->in.rows.numReadChars;
  unsigned malformed = 0;
  for (unsigned long long r = (unsigned long long)blockIdx.x * (kOrientThreads / 64u) + threadIdx.x / 64u; r < R; r += numWaves) {
    asm volatile("" : "+s"(q));
    const unsigned long long base = offsets[0], f0 = offsets[r], f1 = offsets[r + 1ull], v0 = offsets[R + r], v1 = offsets[R + r + 1ull];
    const unsigned strand = q->in.strands[r];
    const unsigned long long n = f1 - f0, to = f0 - base;
    /* (the same in every lane) */
    const bool good = f0 <= f1 && f1 <= numChars && v0 <= v1 && v1 <= numChars && v1 - v0 == n && strand <= 1u && f0 >= base && f1 - base <= q->out.capacity;
    if (lane == 0u) {
      q->out.readOffsets[r] = to;
      if (r + 1ull == R) q->out.readOffsets[R] = f1 - base;
      malformed += good ? 0u : 1u;
    }
    if (good) {
      orientCopy(q->in.rows.readChars, numChars, strand ? v0 : f0, q->out.readChars + to, (long long)n, false, lane);
      if (q->out.qualities) orientCopy(q->in.qualities, numChars, f0, q->out.qualities + to, (long long)n, strand != 0u, lane);
    }
    if (lane < q->slots) {
      const unsigned long long at = r * q->slots + lane, source = (good ? (strand ? R : 0ull) + r : 0ull) * q->slots + lane;
      if (q->out.sequences) q->out.sequences[at] = good ? q->in.rows.sequences[source] : AWFM_CANDIDATES_NONE;
      if (q->out.chainAnchors) q->out.chainAnchors[at] = good ? q->in.rows.chainAnchors[source] : 0u;
      if (q->out.chainReadBegins) q->out.chainReadBegins[at] = good ? q->in.rows.chainReadBegins[source] : 0u;
      if (q->out.chainReadEnds) q->out.chainReadEnds[at] = good ? q->in.rows.chainReadEnds[source] : 0u;
      if (q->out.chainBeginDiagonals) q->out.chainBeginDiagonals[at] = good ? q->in.rows.chainBeginDiagonals[source] : 0ll;
      if (q->out.chainEndDiagonals) q->out.chainEndDiagonals[at] = good ? q->in.rows.chainEndDiagonals[source] : 0ll;
      if (q->out.slotScores) q->out.slotScores[at] = good ? q->in.slotScores[source] : AWFM_VERIFY_NONE;
      if (q->out.slotReadEnds) q->out.slotReadEnds[at] = good ? q->in.slotReadEnds[source] : 0u;
      if (q->out.slotTextEnds) q->out.slotTextEnds[at] = good ? q->in.slotTextEnds[source] : 0ull;
    }
  }
  if (lane == 0u && malformed && q->out.numMalformed) atomicAdd((unsigned long long *)q->out.numMalformed, (unsigned long long)malformed);
}

}  // namespace

#endif
