/*
 * awfm_chains_kernel.h -- the best colinear chain of every candidate slot of every read on the device: the kernels of
 * awfmGpuReadChains (definition: include/awfm_gpu.h, "read chains"; host twin: awfm_chains.c).  The reference has no analogue (it
 * stops at positions: ref src/AwFmParallelSearch.c:315-365).
 *
 * One routine, chainsOfRead<THREADS, CAP>, does a read with a workgroup of THREADS threads and room for CAP anchors:
 *
 *   check    awfm_hits_kernel.h's, and the read's at most 16 slots against each other (256 pairs): a malformed read is reported
 *            and read no further.  The slots (sequence, diagonal ^ 2^63, span) stay in LDS.
 *   gather   awfm_hits_kernel.h's.  Every kept hit is counted; the one that lies in a slot is an anchor and is appended to LDS as
 *            two 64-bit words, (slot << 32 | e) and ((D - the slot's diagonal) << 32 | len): a slot's interval is at most
 *            2^32 - 1 wide, so the diagonal travels as 32 bits and an anchor is 16 bytes, sort key and payload in one.
 *   sort     bitonic, in LDS, over the next power of two, by those two words: (slot, e, D, len), the definition's order
 *            (padding sorts last).  A neighbour compare then gives every slot its range.
 *   chain    a WAVE per slot, the slots of a read one after another (wave tier) or eight at a time (workgroup tier).  The
 *            recurrence is sequential in the anchor and parallel in the predecessor: lane l keeps, in six registers, what the
 *            last anchor at an order position = l mod 64 carries (e, D, f, and its chain's first a, first D and length), so the
 *            64 lanes are the lookback window.  An anchor's own (e, D, len) comes out of a register of the lane that loaded it
 *            (64 anchors per LDS read) as scalars; each lane values its predecessor; a DPP max-reduction (row_shr 1, 2, 4, 8,
 *            row_bcast 15 and 31) gives the best value, and a ballot of the lanes that hold it, rotated so that the nearest
 *            predecessor is the top bit, gives the largest j among ties -- scores span 32 bits, so a packed (value, nearness)
 *            key would be 64 bits wide and double the reduction; the ballot costs three scalar instructions instead.  The
 *            slot's best chain so far lives in scalars.
 *
 * The two tiers of awfm_hits_kernel.h run it.  readChainsWaveKernel: CAP = kChainsWaveLimit; a read with more anchors (and at
 * most AWFM_CANDIDATES_MAX_HITS kept hits) goes onto the worklist (its gather has then only counted).  readChainsGroupKernel:
 * workgroups of kChainsGroupThreads with CAP = AWFM_CANDIDATES_MAX_HITS: 64 KB of anchors and the slots, beyond the 64 KB a
 * launch gets without asking, hence dynamic LDS (the launch sets the kernel's limit for the device at hand each time); two such
 * workgroups share a CU's 160 KB.  Reads with more kept hits are overflowed: reported by the wave tier, never sorted.
 *
 * Vector loads and stores only; outputs are stored per read in whole runs of slots by the first C threads.
 */
#ifndef AWFM_CHAINS_KERNEL_H
#define AWFM_CHAINS_KERNEL_H

#include <type_traits>

#include "awfm_hits_kernel.h"

namespace {

constexpr unsigned kChainsWaveLimit = 256;    /* anchors a wave sorts by itself: four per lane */
constexpr unsigned kChainsGroupLimit = 4096;  /* = AWFM_CANDIDATES_MAX_HITS */
constexpr unsigned kChainsWaveThreads = 64;   /* per workgroup of the wave tier: one wave */
constexpr unsigned kChainsGroupThreads = 512; /* per workgroup of the workgroup tier: eight waves, a slot each at a time */
constexpr unsigned kChainsEntryBytes = 16;    /* LDS per anchor: slot 4, e 4, relative diagonal 4, len 4 */
constexpr unsigned kChainsWaveLdsBytes = 5376;   /* static LDS of the wave tier's kernel at the most (4096 + slots): 5.25 KB */
constexpr unsigned kChainsGroupLdsBytes = 66560; /* dynamic LDS of the workgroup tier's (65536 + slots): 65 KB, two per CU */
constexpr unsigned kChainsSlots = 16;         /* = AWFM_CANDIDATES_MAX_SLOTS */

static_assert(kChainsGroupLimit == AWFM_CANDIDATES_MAX_HITS && kChainsSlots == AWFM_CANDIDATES_MAX_SLOTS, "include/awfm_gpu.h");
static_assert(AWFM_CHAINS_MAX_LOOKBACK == 64u, "the lookback window is the 64 lanes of a wave");
static_assert(2u * kChainsGroupLdsBytes <= 160u * 1024u, "two workgroups of the workgroup tier per CU");

struct DevChainParams {
  AwFmCandidateInputs in;
  AwFmChainOutputs out;
  const unsigned *sequences; /* the slots: [numReads * slots] */
  const long long *diagonals;
  const unsigned *spans;
  unsigned long long numReads;
  unsigned maxHitsPerSeed, band, slots, lookback, gapPenalty;
  unsigned waveLimit;          /* anchors up to which the wave tier does a read itself (0: every read with one goes to the worklist) */
  unsigned long long *counter; /* dScratch: the worklist's length ... */
  unsigned *worklist;          /* ... and its numReads entries */
};

/* LDS of one workgroup */
template <unsigned CAP>
struct ChainsLds {
  unsigned long long hi[CAP]; /* slot << 32 | e */
  unsigned long long lo[CAP]; /* (D - the slot's diagonal) << 32 | len */
  unsigned long long kept;    /* the true number of kept hits in the end */
  unsigned long long slotLow[kChainsSlots]; /* the slot's diagonal ^ 2^63 */
  unsigned slotSequence[kChainsSlots], slotSpan[kChainsSlots];
  unsigned slotBegin[kChainsSlots], slotEnd[kChainsSlots]; /* the slot's anchors once they are sorted */
  unsigned score[kChainsSlots], anchors[kChainsSlots], readBegin[kChainsSlots], readEnd[kChainsSlots]; /* the slot's best chain */
  unsigned beginDiagonal[kChainsSlots], endDiagonal[kChainsSlots];                                     /* (relative) */
  unsigned numAnchors; /* appended so far: runs on beyond CAP */
};
static_assert(sizeof(ChainsLds<kChainsWaveLimit>) <= kChainsWaveLdsBytes, "the wave tier's LDS");
static_assert(sizeof(ChainsLds<kChainsGroupLimit>) <= kChainsGroupLdsBytes, "the workgroup tier's LDS");

/* the largest v of the wave's 64 lanes, in every lane: DPP within the rows of 16, the rows' last lanes broadcast onwards */
__device__ __forceinline__ unsigned waveMax(unsigned v) {
  auto step = [](unsigned x, unsigned moved) { return moved > x ? moved : x; };
  /* (a lane without a source, or outside the row mask, receives `old` = 0: the identity) */
  v = step(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, false)); /* row_shr:1 */
  v = step(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, false)); /* row_shr:2 */
  v = step(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, false)); /* row_shr:4 */
  v = step(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, false)); /* row_shr:8: lane 15 of a row has the row */
  v = step(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false)); /* row_bcast:15 into rows 1 and 3 */
  v = step(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false)); /* row_bcast:31 into rows 2 and 3 */
  return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

/* The recurrence over slot j's anchors, by the calling wave; the slot's best chain is left in LDS by lane 0. */
template <unsigned CAP>
__device__ __forceinline__ void chainSlot(const DevChainParams &p, ChainsLds<CAP> &s, unsigned j) {
  const unsigned lane = threadIdx.x & 63u;
  const unsigned begin = (unsigned)__builtin_amdgcn_readfirstlane((int)s.slotBegin[j]);
  const unsigned end = (unsigned)__builtin_amdgcn_readfirstlane((int)s.slotEnd[j]);
  if (begin >= end) return; /* (the slot's results are zero already) */
  /* what the last anchor at an order position = lane (mod 64) carries */
  unsigned prevEnd = 0u, prevDiagonal = 0u, prevScore = 0u, prevBegin = 0u, prevBeginDiagonal = 0u, prevAnchors = 0u;
  /* the best chain so far (wave-uniform) */
  unsigned bestScore = 0u, bestAnchors = 0u, bestBegin = 0u, bestEnd = 0u, bestBeginDiagonal = 0u, bestEndDiagonal = 0u;
  for (unsigned base = begin; base < end; base += 64u) {
    const unsigned mine = base + lane;
    const unsigned long long hi = mine < end ? s.hi[mine] : 0ull, lo = mine < end ? s.lo[mine] : 0ull;
    const unsigned myEnd = (unsigned)hi, myDiagonal = (unsigned)(lo >> 32), myLength = (unsigned)lo;
    const unsigned count = end - base < 64u ? end - base : 64u;
    for (unsigned t = 0; t < count; t++) {
      const unsigned e = (unsigned)__builtin_amdgcn_readlane((int)myEnd, (int)t);
      const unsigned d = (unsigned)__builtin_amdgcn_readlane((int)myDiagonal, (int)t);
      const unsigned length = (unsigned)__builtin_amdgcn_readlane((int)myLength, (int)t);
      const unsigned position = base - begin + t; /* in the slot's order; lane `position & 63` takes this anchor in the end */
      const unsigned distance = ((position - 1u - lane) & 63u) + 1u; /* to the anchor this lane holds, if it holds one */
      const unsigned reach = position < p.lookback ? position : p.lookback;
      const long long dr = (long long)e - (long long)prevEnd, dd = (long long)d - (long long)prevDiagonal, dt = dr + dd;
      const unsigned long long gap = (unsigned long long)(dd < 0 ? -dd : dd);
      unsigned value = 0u;
      if (distance <= reach && dr > 0 && dt > 0 && gap <= p.band) {
        long long step = dr < dt ? dr : dt;
        step = step < (long long)length ? step : (long long)length;
        const unsigned long long gain = (unsigned long long)prevScore + (unsigned long long)step, penalty = gap * p.gapPenalty;
        /* (gain - penalty <= e: 32 bits hold it) */
        if (gain > penalty && gain - penalty > length) value = (unsigned)(gain - penalty);
      }
      const unsigned best = waveMax(value);
      unsigned score = length, first = e - length, firstDiagonal = d, anchors = 1u;
      if (best != 0u) { /* (uniform) among the lanes that hold the best value, the nearest: the largest order position */
        const unsigned long long holders = __ballot(value == best);
        const unsigned top = (position - 1u) & 63u, turn = 63u - top; /* lane `top` is at distance 1: turn it to bit 63 */
        const unsigned long long turned = turn ? (holders << turn) | (holders >> (64u - turn)) : holders;
        const unsigned winner = ((63u - (unsigned)__clzll((long long)turned)) + top + 1u) & 63u;
        score = best;
        first = (unsigned)__builtin_amdgcn_readlane((int)prevBegin, (int)winner);
        firstDiagonal = (unsigned)__builtin_amdgcn_readlane((int)prevBeginDiagonal, (int)winner);
        anchors = (unsigned)__builtin_amdgcn_readlane((int)prevAnchors, (int)winner) + 1u;
      }
      if (lane == (position & 63u)) {
        prevEnd = e;
        prevDiagonal = d;
        prevScore = score;
        prevBegin = first;
        prevBeginDiagonal = firstDiagonal;
        prevAnchors = anchors;
      }
      if (bestAnchors == 0u || score > bestScore) { /* (ties: the smallest order position) */
        bestScore = score;
        bestAnchors = anchors;
        bestBegin = first;
        bestEnd = e;
        bestBeginDiagonal = firstDiagonal;
        bestEndDiagonal = d;
      }
    }
  }
  if (lane == 0u) {
    s.score[j] = bestScore;
    s.anchors[j] = bestAnchors;
    s.readBegin[j] = bestBegin;
    s.readEnd[j] = bestEnd;
    s.beginDiagonal[j] = bestBeginDiagonal;
    s.endDiagonal[j] = bestEndDiagonal;
  }
}

/* Read r's slots, best slot and kept hits from what LDS holds (all zero and none for a read without chains of its own).  The
 * outputs, and the slot arrays in chainsOfRead, where they are used, not before (kernelArguments): the kernels' arguments are 54
 * words, and the recurrence spills scalar registers when they are loaded ahead of the loop over the reads. */
template <unsigned CAP>
__device__ __forceinline__ void storeChains(const DevChainParams &p, const ChainsLds<CAP> &s, unsigned long long r, bool chained,
                                            unsigned keptHits) {
  const auto &out = kernelArguments<DevChainParams>()->out;
  const unsigned j = threadIdx.x;
  if (j < p.slots) {
    const unsigned long long at = r * p.slots + j;
    const bool has = chained && s.anchors[j] != 0u;
    if (out.chainScores) out.chainScores[at] = has ? s.score[j] : 0u;
    if (out.chainAnchors) out.chainAnchors[at] = has ? s.anchors[j] : 0u;
    if (out.chainReadBegins) out.chainReadBegins[at] = has ? s.readBegin[j] : 0u;
    if (out.chainReadEnds) out.chainReadEnds[at] = has ? s.readEnd[j] : 0u;
    if (out.chainBeginDiagonals) out.chainBeginDiagonals[at] = has ? (long long)((s.slotLow[j] + s.beginDiagonal[j]) ^ kHitsSign) : 0ll;
    if (out.chainEndDiagonals) out.chainEndDiagonals[at] = has ? (long long)((s.slotLow[j] + s.endDiagonal[j]) ^ kHitsSign) : 0ll;
  }
  if (j == 0u) {
    unsigned bestSlot = kHitsNone, bestScore = 0u;
    if (chained)
      for (unsigned k = 0; k < p.slots; k++)
        if (s.anchors[k] != 0u && (bestSlot == kHitsNone || s.score[k] > bestScore)) {
          bestSlot = k;
          bestScore = s.score[k];
        }
    if (out.bestSlots) out.bestSlots[r] = bestSlot;
    if (out.keptHits) out.keptHits[r] = keptHits;
    if (!chained && out.numOverflowed) atomicAdd((unsigned long long *)out.numOverflowed, 1ull);
  }
}

/* Read r by the calling workgroup.  Returns true when the read has more than `limit` (<= CAP) anchors and at most
 * AWFM_CANDIDATES_MAX_HITS kept hits: nothing was stored, the read is the other tier's.  Workgroup-uniform. */
template <unsigned THREADS, unsigned CAP>
__device__ bool chainsOfRead(const DevChainParams &p, ChainsLds<CAP> &s, unsigned long long r, unsigned limit) {
  static_assert(CAP % THREADS == 0 && (CAP & (CAP - 1u)) == 0, "a power of two, whole rounds");
  constexpr unsigned kWaves = THREADS / 64u;
  const unsigned tid = threadIdx.x;
  __syncthreads(); /* the LDS of the read before */
  if (tid == 0u) {
    s.kept = 0ull;
    s.numAnchors = 0u;
  }
  if (tid < kChainsSlots) {
    const auto params = kernelArguments<DevChainParams>();
    const bool used = tid < p.slots;
    s.slotSequence[tid] = used ? params->sequences[r * p.slots + tid] : kHitsNone;
    s.slotLow[tid] = used ? (unsigned long long)params->diagonals[r * p.slots + tid] ^ kHitsSign : 0ull;
    s.slotSpan[tid] = used ? params->spans[r * p.slots + tid] : 0u;
    s.slotBegin[tid] = 0u;
    s.slotEnd[tid] = 0u;
    s.anchors[tid] = 0u;
  }
  /* check */
  unsigned long long seedBegin, seedEnd;
  bool malformed = __syncthreads_or(readMalformed<THREADS>(p.in, r, seedBegin, seedEnd));
  if (!malformed) { /* two slots of one sequence whose intervals intersect */
    bool intersect = false;
    for (unsigned q = tid; q < kChainsSlots * kChainsSlots; q += THREADS) {
      const unsigned a = q / kChainsSlots, b = q % kChainsSlots;
      if (a >= b || s.slotSequence[a] == kHitsNone || s.slotSequence[a] != s.slotSequence[b]) continue;
      const unsigned long long lowA = s.slotLow[a], lowB = s.slotLow[b];
      const unsigned long long highA = lowA + s.slotSpan[a] < lowA ? ~0ull : lowA + s.slotSpan[a];
      const unsigned long long highB = lowB + s.slotSpan[b] < lowB ? ~0ull : lowB + s.slotSpan[b];
      intersect |= lowA <= highB && lowB <= highA;
    }
    malformed = __syncthreads_or(intersect);
  }
  if (malformed) {
    storeChains(p, s, r, false, kHitsMalformed);
    return false;
  }
  /* gather */
  unsigned long long low, high;
  wavePart<THREADS>(p.in, seedBegin, seedEnd, low, high);
  visitHits(p,seedBegin, seedEnd, low, high, [&](bool keep, unsigned sequence, unsigned long long key, unsigned anchor, unsigned end) {
    const unsigned long long keptMask = __ballot(keep);
    if (keptMask == 0ull) return;
    unsigned slot = kHitsNone;
    if (keep)
      for (unsigned j = 0; j < p.slots; j++)
        if (s.slotSequence[j] == sequence && key >= s.slotLow[j] && key - s.slotLow[j] <= s.slotSpan[j]) slot = j; /* (at most one) */
    const unsigned long long mask = __ballot(slot != kHitsNone);
    const int leader = __ffsll((long long)keptMask) - 1;
    (void)waveAppend(&s.kept, keptMask, leader);
    const unsigned at = waveAppend(&s.numAnchors, mask, leader);
    if (slot != kHitsNone && at < CAP) {
      s.hi[at] = ((unsigned long long)slot << 32) | end;
      s.lo[at] = ((key - s.slotLow[slot]) << 32) | (end - anchor);
    }
  });
  __syncthreads();
  const unsigned long long kept = s.kept;
  if (kept > kChainsGroupLimit) {
    storeChains(p, s, r, false, keptHitsWord(kept));
    return false;
  }
  const unsigned n = s.numAnchors; /* <= kept */
  if (n > limit) return true;
  /* sort: by (hi, lo) */
  struct Anchor {
    unsigned long long hi, lo;
  };
  sortLds<THREADS>(
      n, Anchor{~0ull, ~0ull}, [&](unsigned i) { return Anchor{s.hi[i], s.lo[i]}; },
      [&](unsigned i, const Anchor &x) {
        s.hi[i] = x.hi;
        s.lo[i] = x.lo;
      },
      [](const Anchor &x, const Anchor &y) { return x.hi != y.hi ? x.hi > y.hi : x.lo > y.lo; });
  /* the slots' ranges */
  for (unsigned i = tid; i < n; i += THREADS) {
    const unsigned slot = (unsigned)(s.hi[i] >> 32);
    if (i == 0u || (unsigned)(s.hi[i - 1u] >> 32) != slot) s.slotBegin[slot] = i;
    if (i + 1u == n || (unsigned)(s.hi[i + 1u] >> 32) != slot) s.slotEnd[slot] = i + 1u;
  }
  __syncthreads();
  /* chain: a wave per slot */
  for (unsigned j = tid >> 6; j < p.slots; j += kWaves) chainSlot(p, s, j);
  __syncthreads();
  storeChains(p, s, r, true, (unsigned)kept);
  return false;
}

/* the wave tier: what it cannot hold goes onto the worklist */
__global__ void __launch_bounds__(kChainsWaveThreads) readChainsWaveKernel(const DevChainParams p) {
  __shared__ ChainsLds<kChainsWaveLimit> s;
  waveTier(p, blockIdx.x, gridDim.x, [&](unsigned long long r) { return chainsOfRead<kChainsWaveThreads, kChainsWaveLimit>(p, s, r, p.waveLimit); });
}

/* the workgroup tier; its LDS is dynamic (kChainsGroupLdsBytes) */
__global__ void __launch_bounds__(kChainsGroupThreads) readChainsGroupKernel(const DevChainParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char chainsGroupLds[];
  ChainsLds<kChainsGroupLimit> &s = *reinterpret_cast<ChainsLds<kChainsGroupLimit> *>(chainsGroupLds);
  groupTier(p, blockIdx.x, gridDim.x, [&](unsigned long long r) { return chainsOfRead<kChainsGroupThreads, kChainsGroupLimit>(p, s, r, kChainsGroupLimit); });
}

/* kernelArguments() reads the argument segment as a DevChainParams: right only while that struct is the one argument of both
 * kernels, by value, hence at offset 0.  A change of either signature stops the build here. */
static_assert(std::is_same<decltype(&readChainsWaveKernel), void (*)(DevChainParams)>::value &&
                  std::is_same<decltype(&readChainsGroupKernel), void (*)(DevChainParams)>::value,
              "kernelArguments() assumes DevChainParams is the kernels' only argument");

}  // namespace

#endif
