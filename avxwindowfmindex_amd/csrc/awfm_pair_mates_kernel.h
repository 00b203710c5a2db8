/*
 * awfm_pair_mates_kernel.h -- pairMatesKernel<G> and reverseComplementKernel, the kernels of "pair mates" (include/awfm_gpu.h).
 * The definition is the header's; the host twin and checker is awfm_pair_mates.c.
 *
 * PAIRING.  A group of G lanes takes a pair (persistent grid over pairs, 64 / G pairs a wave in step), lane k of the group holds
 * slot a = k / 4 of mate A and the slots b = k % 4 + 4 t of mate B, t < Q: Q = 1 at G = 16 (C <= 4: a lane per (a, b)), Q = 4 at
 * G = 64 (C <= 16).  Each lane loads its slots ONCE -- score, read end, text end, sequence -- and the pair's three read offsets;
 * everything after that is registers and cross-lane moves: no LDS, no atomics but the two counters.  Three keyed 64-bit maxima
 * over the group (a butterfly of __shfl_xor each, so every lane ends with the result):
 *   both bests   (score_A + 1 where A's slot counts) + (the same of B), then "A counts", "B counts", 15 - a, 15 - b.  The sum is
 *                largest exactly at (best(A), best(B)) -- each addend at its own maximum, ties to the lowest a, then b, which is
 *                each mate's lowest slot -- so ONE maximum yields both best slots and whether each mate has one.
 *   the winner   exists, value, concordant, 15 - a, 15 - b over the lane's candidates: the concordant ones, and the discordant
 *                one in the lane that holds (best(A), best(B)); the header's tie rule is the comparison itself.
 *   the second   the same keys with the winner's duplicates masked out (the winner among them: j' = j).
 * Between the last two the winner's slots -- or, without a winner, what bests there are -- come to every lane by __shfl from the
 * lanes that hold them (five words a mate): the duplicate test, the single mate's score and the windows read them there.  Lane 0
 * of a group stores the pair's outputs and read A's, lane 1 read B's.  The quality's division is 32-bit whenever every group of
 * the wave has cap * win below 2^32 (a wave-uniform branch; always, for scores the library wrote), else 64-bit.
 *
 * THE INTERVAL is the launch's, or -- awfmGpuPairMatesEstimated, "insert size" -- the one an earlier kernel of the stream left in
 * a struct AwFmInsertEstimate: one uniform pointer in the parameters, read once at the top of the kernel together with a uniform
 * "usable" flag (the host has not seen that interval, so the kernel validates it), which gates "concordant" and the windows.  The
 * same two instantiations serve both calls.
 *
 * REVERSE COMPLEMENT.  A wave per read, a lane per ALIGNED word of the output (aligned as an address, so the read's first and
 * last word may be partial and are stored bytewise).  The four source bytes of a word -- the mirrored ones of a selected read,
 * the same ones of a copied read -- lie anywhere: one or two aligned words of the input, each loaded only when it holds a byte of
 * the buffer, funnelled by v_alignbyte.  Vector loads and stores only.
 */
#ifndef AWFM_PAIR_MATES_KERNEL_H
#define AWFM_PAIR_MATES_KERNEL_H

#include "awfm_device.h"

namespace {

constexpr unsigned kPairThreads = 256;   /* per workgroup: four waves */
constexpr unsigned kPairBlocksPerCU = 4; /* up to 128 VGPRs: four waves per SIMD, i.e. four workgroups of four waves per CU */
constexpr unsigned kPairMaxVgprs = 128;
constexpr unsigned kPairLdsBytes = 0;    /* no LDS */

struct DevPairParams {
  struct AwFmPairInputs in;
  struct AwFmPairOutputs out;
  unsigned long long numPairs;
  long long minInsert, maxInsert, pad;
  unsigned slots, floor, penalty, cap; /* floor: max(minScore, 1) */
  const struct AwFmInsertEstimate *estimate; /* awfmGpuPairMatesEstimated: the interval lies there; NULL: minInsert, maxInsert above */
};

struct DevComplementParams {
  const unsigned char *chars;
  unsigned char *out;
  const unsigned long long *offsets;
  unsigned long long numChars, numReads;
  unsigned long long *numMalformed;
  unsigned which;
};

template <int G>
__device__ __forceinline__ unsigned long long pairGroupMax(unsigned long long key) {
#pragma unroll
  for (int step = 1; step < G; step <<= 1) {
    const unsigned otherLow = (unsigned)__shfl_xor((int)(unsigned)key, step, G), otherHigh = (unsigned)__shfl_xor((int)(unsigned)(key >> 32), step, G);
    const unsigned long long other = ((unsigned long long)otherHigh << 32) | otherLow;
    key = other > key ? other : key;
  }
  return key;
}

/* what the lane that holds slot b of mate B has of it: lane b % 4 of the group, its register b / 4 */
template <int G, int Q>
__device__ __forceinline__ unsigned pairFromB(const unsigned (&mine)[Q], const unsigned b) {
  unsigned chosen = mine[0];
#pragma unroll
  for (int t = 1; t < Q; t++) chosen = (b >> 2) == (unsigned)t ? mine[t] : chosen;
  return (unsigned)__shfl((int)chosen, (int)(b & 3u), G);
}

/* the launch's parameters where the launch left them, in the kernel's argument segment: a field is loaded where it is used
 * instead of living in a register from the kernel's first instruction to its last (scoreChainsAffineKernel does the same) */
typedef const __attribute__((address_space(4))) DevPairParams *PairParamsRef;

constexpr unsigned long long kPairKeyExists = 1ull << 42; /* value < 2^33 above concordant << 8 | 15 - a << 4 | 15 - b */

template <int G>
__global__ void __launch_bounds__(kPairThreads, 4) pairMatesKernel(const DevPairParams args) {
  (void)args; /* (the struct is the kernel's only argument, so it begins the segment) */
  PairParamsRef p = (PairParamsRef)__builtin_amdgcn_kernarg_segment_ptr();
  constexpr int Q = G == 64 ? 4 : 1;
  constexpr unsigned kGroupsPerBlock = kPairThreads / (unsigned)G;
  const unsigned lane = threadIdx.x & 63u, k = lane % (unsigned)G, a = k >> 2;
  const unsigned C = p->slots;
  /* the interval: the launch's, or the one an earlier kernel of the stream left in device memory ("insert size"), which nobody
   * has validated: one that is not usable makes no pair concordant and names no window (uniform, like the interval itself) */
  long long minInsert = p->minInsert, maxInsert = p->maxInsert;
  bool usable = true;
  if (p->estimate) {
    minInsert = p->estimate->minInsert;
    maxInsert = p->estimate->maxInsert;
    usable = minInsert <= maxInsert && minInsert >= -AWFM_PAIR_MAX_INSERT && maxInsert <= AWFM_PAIR_MAX_INSERT;
  }
  const unsigned long long stride = (unsigned long long)gridDim.x * kGroupsPerBlock;
  /* every group of a wave makes the same number of trips: the cross-lane moves want the whole wave */
  const unsigned long long waveFirst = (unsigned long long)blockIdx.x * kGroupsPerBlock + (threadIdx.x / 64u) * (64u / (unsigned)G);
  unsigned proper = 0, windows = 0;
  for (unsigned long long first = waveFirst; first < p->numPairs; first += stride) {
    asm volatile("" : "+s"(p));
    const unsigned long long pair = first + lane / (unsigned)G;
    const bool active = pair < p->numPairs;
    const unsigned long long A = 2ull * pair;
    unsigned long long o0 = 0, o1 = 0, o2 = 0;
    if (active) {
      o0 = p->in.readOffsets[A];
      o1 = p->in.readOffsets[A + 1ull];
      o2 = p->in.readOffsets[A + 2ull];
    }
    const long long nA = (long long)(o1 - o0), nB = (long long)(o2 - o1);
    /* the lane's slots */
    unsigned scoreA = 0, seqA = 0, endA = 0, textLowA = 0, textHighA = 0;
    bool countsA = false;
    if (active && a < C) {
      const unsigned long long at = A * C + a;
      scoreA = p->in.slotScores[at];
      seqA = p->in.sequences[at];
      endA = p->in.slotReadEnds[at];
      const unsigned long long textEnd = p->in.slotTextEnds[at];
      textLowA = (unsigned)textEnd;
      textHighA = (unsigned)(textEnd >> 32);
      countsA = o0 <= o1 && scoreA < AWFM_VERIFY_TOO_LONG && scoreA >= p->floor;
    }
    const long long startA = (long long)((((unsigned long long)textHighA << 32) | textLowA) - endA);
    unsigned scoreB[Q], seqB[Q], endB[Q], textLowB[Q], textHighB[Q];
    bool countsB[Q];
#pragma unroll
    for (int t = 0; t < Q; t++) {
      const unsigned b = (k & 3u) + 4u * (unsigned)t;
      scoreB[t] = seqB[t] = endB[t] = textLowB[t] = textHighB[t] = 0u;
      countsB[t] = false;
      if (active && b < C) {
        const unsigned long long at = (A + 1ull) * C + b;
        scoreB[t] = p->in.slotScores[at];
        seqB[t] = p->in.sequences[at];
        endB[t] = p->in.slotReadEnds[at];
        const unsigned long long textEnd = p->in.slotTextEnds[at];
        textLowB[t] = (unsigned)textEnd;
        textHighB[t] = (unsigned)(textEnd >> 32);
        countsB[t] = o1 <= o2 && scoreB[t] < AWFM_VERIFY_TOO_LONG && scoreB[t] >= p->floor;
      }
    }
    /* both bests in one maximum */
    unsigned long long bestsKey = 0;
#pragma unroll
    for (int t = 0; t < Q; t++) {
      const unsigned b = (k & 3u) + 4u * (unsigned)t;
      const unsigned long long sum = (countsA ? (unsigned long long)scoreA + 1ull : 0ull) + (countsB[t] ? (unsigned long long)scoreB[t] + 1ull : 0ull);
      const unsigned long long key = (sum << 10) | (countsA ? 512ull : 0ull) | (countsB[t] ? 256ull : 0ull) | ((15u - a) << 4) | (15u - b);
      bestsKey = active && a < C && b < C && key > bestsKey ? key : bestsKey;
    }
    bestsKey = pairGroupMax<G>(bestsKey);
    const bool hasA = (bestsKey & 512ull) != 0, hasB = (bestsKey & 256ull) != 0;
    const unsigned bestA = 15u - ((unsigned)(bestsKey >> 4) & 15u), bestB = 15u - ((unsigned)bestsKey & 15u);
    /* the lane's candidates */
    unsigned long long keys[Q], winnerKey = 0;
    long long lengths[Q];
#pragma unroll
    for (int t = 0; t < Q; t++) {
      const unsigned b = (k & 3u) + 4u * (unsigned)t;
      const long long startB = (long long)((((unsigned long long)textHighB[t] << 32) | textLowB[t]) - endB[t]);
      const long long T = (long long)((unsigned long long)startB + (unsigned long long)nB - (unsigned long long)startA);
      const bool both = countsA && countsB[t];
      const bool concordant = both && usable && seqA == seqB[t] && minInsert <= T && T <= maxInsert;
      unsigned long long value = (unsigned long long)scoreA + scoreB[t];
      bool exists = concordant;
      if (both && !concordant && hasA && hasB && a == bestA && b == bestB) {
        exists = true;
        value = value > p->penalty ? value - p->penalty : 0ull;
      }
      keys[t] = exists ? kPairKeyExists | (value << 9) | (concordant ? 256ull : 0ull) | ((15u - a) << 4) | (15u - b) : 0ull;
      lengths[t] = T;
      winnerKey = keys[t] > winnerKey ? keys[t] : winnerKey;
    }
    winnerKey = pairGroupMax<G>(winnerKey);
    const bool hasWinner = winnerKey != 0, isProper = (winnerKey & 256ull) != 0;
    const unsigned slotA = hasWinner ? 15u - ((unsigned)(winnerKey >> 4) & 15u) : bestA, slotB = hasWinner ? 15u - ((unsigned)winnerKey & 15u) : bestB;
    /* the chosen slots, in every lane (slot 15 of a mate that has none: read and not used) */
    const int holderA = (int)(slotA << 2) & (G - 1);
    const unsigned chosenScoreA = (unsigned)__shfl((int)scoreA, holderA, G), chosenSeqA = (unsigned)__shfl((int)seqA, holderA, G);
    const unsigned chosenEndA = (unsigned)__shfl((int)endA, holderA, G), chosenLowA = (unsigned)__shfl((int)textLowA, holderA, G);
    const unsigned chosenHighA = (unsigned)__shfl((int)textHighA, holderA, G);
    const unsigned chosenScoreB = pairFromB<G, Q>(scoreB, slotB), chosenSeqB = pairFromB<G, Q>(seqB, slotB);
    const unsigned chosenEndB = pairFromB<G, Q>(endB, slotB), chosenLowB = pairFromB<G, Q>(textLowB, slotB);
    const unsigned chosenHighB = pairFromB<G, Q>(textHighB, slotB);
    /* the second: the winner's duplicates masked out (both of the winner's slots count) */
    const bool sameA = a == slotA || (countsA && seqA == chosenSeqA && endA == chosenEndA && textLowA == chosenLowA && textHighA == chosenHighA);
    unsigned long long secondKey = 0;
    long long length = 0;
#pragma unroll
    for (int t = 0; t < Q; t++) {
      const unsigned b = (k & 3u) + 4u * (unsigned)t;
      const bool sameB = b == slotB || (countsB[t] && seqB[t] == chosenSeqB && endB[t] == chosenEndB && textLowB[t] == chosenLowB && textHighB[t] == chosenHighB);
      const unsigned long long key = sameA && sameB ? 0ull : keys[t];
      secondKey = key > secondKey ? key : secondKey;
      length = keys[t] == winnerKey ? lengths[t] : length; /* (the lane that holds the winner) */
    }
    secondKey = pairGroupMax<G>(secondKey);
    /* T of the winner from the lane that holds it: lane a << 2 | b % 4 */
    const int holder = (int)((slotA << 2) | (slotB & 3u)) & (G - 1);
    const unsigned lengthLow = (unsigned)__shfl((int)(unsigned)(unsigned long long)length, holder, G);
    const unsigned lengthHigh = (unsigned)__shfl((int)(unsigned)((unsigned long long)length >> 32), holder, G);
    const unsigned long long win = (winnerKey >> 9) & 0x1FFFFFFFFull, second = (secondKey >> 9) & 0x1FFFFFFFFull;
    /* 6: the division in 32 bits where every group of the wave allows it */
    const unsigned long long numerator = isProper ? (unsigned long long)p->cap * (win - second) : 0ull, denominator = isProper ? win : 1ull;
    unsigned quality;
    if (__builtin_amdgcn_ballot_w64((numerator | denominator) >> 32 != 0ull) == 0ull) quality = (unsigned)numerator / (unsigned)denominator;
    else quality = (unsigned)(numerator / denominator);
    unsigned long long value = win;
    if (!hasWinner) value = hasA ? chosenScoreA : hasB ? chosenScoreB : 0u;
    if (active && k == 0u) {
      proper += isProper ? 1u : 0u;
      if (p->out.properPairs) p->out.properPairs[pair] = isProper ? 1 : 0;
      if (p->out.pairScores) p->out.pairScores[pair] = (unsigned)value;
      if (p->out.pairSecondScores) p->out.pairSecondScores[pair] = (unsigned)second;
      if (p->out.templateLengths) p->out.templateLengths[pair] = isProper ? (long long)(((unsigned long long)lengthHigh << 32) | lengthLow) : 0ll;
      if (p->out.pairQualities) p->out.pairQualities[pair] = (unsigned char)quality;
    }
    if (active && k < 2u) { /* lane 0: read A, lane 1: read B */
      const bool isB = k == 1u;
      const unsigned long long r = A + k;
      const bool placed = isB ? hasB : hasA, matePlaced = isB ? hasA : hasB;
      const unsigned chosen = hasWinner || placed ? (isB ? slotB : slotA) : AWFM_CHAINS_NO_SLOT;
      const unsigned given = p->in.mappingQualities ? p->in.mappingQualities[r] : 0u;
      unsigned mine = placed ? given : 0u;
      if (isProper) {
        mine = chosen == (isB ? bestB : bestA) ? given : 0u;
        mine = quality > mine ? quality : mine;
      }
      /* 7: the mate's best slot is the chosen one whenever the pair is not proper */
      unsigned windowSequence = AWFM_CANDIDATES_NONE;
      long long windowBegin = 0, windowEnd = 0;
      if (!isProper && matePlaced && usable) {
        const unsigned long long textEnd = isB ? ((unsigned long long)chosenHighA << 32) | chosenLowA : ((unsigned long long)chosenHighB << 32) | chosenLowB;
        const unsigned long long S = textEnd - (isB ? chosenEndA : chosenEndB);
        windowSequence = isB ? chosenSeqA : chosenSeqB;
        if (isB) {
          windowBegin = (long long)(S + (unsigned long long)minInsert - (unsigned long long)nB - (unsigned long long)p->pad);
          windowEnd = (long long)(S + (unsigned long long)maxInsert + (unsigned long long)p->pad);
        } else {
          const unsigned long long E = S + (unsigned long long)nB;
          windowBegin = (long long)(E - (unsigned long long)maxInsert - (unsigned long long)p->pad);
          windowEnd = (long long)(E - (unsigned long long)minInsert + (unsigned long long)nA + (unsigned long long)p->pad);
        }
        windowBegin = windowBegin < 0 ? 0 : windowBegin;
        windowEnd = windowEnd < 0 ? 0 : windowEnd;
        windows++;
      }
      if (p->out.pairSlots) p->out.pairSlots[r] = chosen;
      if (p->out.mappingQualities) p->out.mappingQualities[r] = (unsigned char)mine;
      if (p->out.windowSequences) p->out.windowSequences[r] = windowSequence;
      if (p->out.windowBegins) p->out.windowBegins[r] = (unsigned long long)windowBegin;
      if (p->out.windowEnds) p->out.windowEnds[r] = (unsigned long long)windowEnd;
    }
  }
  /* one atomic per wave and counter that met any */
#pragma unroll
  for (int offset = 32; offset > 0; offset >>= 1) {
    proper += (unsigned)__shfl_xor((int)proper, offset, 64);
    windows += (unsigned)__shfl_xor((int)windows, offset, 64);
  }
  if (lane == 0u && proper && p->out.numProper) atomicAdd((unsigned long long *)p->out.numProper, (unsigned long long)proper);
  if (lane == 0u && windows && p->out.numWindows) atomicAdd((unsigned long long *)p->out.numWindows, (unsigned long long)windows);
}

constexpr unsigned kComplementThreads = 256;   /* per workgroup: four waves, each with reads of its own */
constexpr unsigned kComplementBlocksPerCU = 8; /* up to 64 VGPRs: eight waves per SIMD */
constexpr unsigned kComplementMaxVgprs = 64;

/* the four bytes [at, at + 4) of the buffer, `at` anywhere from -3 on: from the one or two aligned words that hold them, each
 * loaded only when it holds a byte of the buffer; bytes outside the buffer come as zeros */
__device__ __forceinline__ unsigned complementFour(const unsigned char *chars, const unsigned long long numChars, const long long at) {
  const unsigned shift = (unsigned)((unsigned long long)(uintptr_t)chars + (unsigned long long)at) & 3u;
  const long long first = at - (long long)shift; /* the aligned word that holds byte `at` */
  unsigned low = 0u, high = 0u;
  if (first + 4 > 0 && first < (long long)numChars) low = *(const unsigned *)(chars + first);
  if (shift != 0u && first + 8 > 0 && first + 4 < (long long)numChars) high = *(const unsigned *)(chars + first + 4);
  return __builtin_amdgcn_alignbyte(high, low, shift);
}

/* the complement of four packed bytes: A <-> T (an exclusive or with 0x15) and C <-> G (with 0x04) in either case */
__device__ __forceinline__ unsigned complementOfFour(const unsigned word) {
  unsigned result = 0u;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const unsigned c = (word >> (8 * i)) & 0xFFu, upper = c & 0xDFu;
    const unsigned flip = upper == 0x41u || upper == 0x54u ? 0x15u : upper == 0x43u || upper == 0x47u ? 0x04u : 0u;
    result |= (c ^ flip) << (8 * i);
  }
  return result;
}

__global__ void __launch_bounds__(kComplementThreads, 8) reverseComplementKernel(const DevComplementParams p) {
  const unsigned lane = threadIdx.x & 63u;
  const unsigned long long numWaves = (unsigned long long)gridDim.x * (kComplementThreads / 64u);
  unsigned malformed = 0;
  for (unsigned long long r = (unsigned long long)blockIdx.x * (kComplementThreads / 64u) + threadIdx.x / 64u; r < p.numReads; r += numWaves) {
    const unsigned long long readBegin = p.offsets[r], readEnd = p.offsets[r + 1ull];
    if (readBegin > readEnd || readEnd > p.numChars) { /* (the same in every lane) */
      malformed++;
      continue;
    }
    if (!p.out) continue;
    const bool selected = p.which == AWFM_COMPLEMENT_ALL || (p.which == AWFM_COMPLEMENT_ODD) == ((r & 1ull) != 0ull);
    const long long n = (long long)(readEnd - readBegin);
    /* the aligned words of the output that hold a byte of the read: the first begins `lead` bytes before the read */
    const long long lead = (long long)(((unsigned long long)(uintptr_t)p.out + readBegin) & 3ull);
    const long long numWords = (n + lead + 3) >> 2;
    for (long long w = lane; w < numWords; w += 64) {
      const long long i = 4 * w - lead; /* the word's first byte as a position of the read: -3 .. n - 1 */
      /* a selected read: positions n - 4 - i .. n - 1 - i mirrored; a copied one: positions i .. i + 3 */
      unsigned word = complementFour(p.chars, p.numChars, (long long)readBegin + (selected ? n - 4 - i : i));
      if (selected) word = complementOfFour(__builtin_bswap32(word));
      unsigned char *to = p.out + ((long long)readBegin + i);
      if (i >= 0 && i + 4 <= n) {
        *(unsigned *)to = word;
      } else {
#pragma unroll
        for (int b = 0; b < 4; b++)
          if (i + b >= 0 && i + b < n) to[b] = (unsigned char)(word >> (8 * b));
      }
    }
  }
  if (lane == 0u && malformed && p.numMalformed) atomicAdd(p.numMalformed, (unsigned long long)malformed);
}

}  // namespace

#endif
