/*
 * awfm_candidates_kernel.h -- the located seeds of a read grouped into candidate loci on the device: the kernels of
 * awfmGpuReadCandidates (definition: include/awfm_gpu.h, "candidate loci"; host twin: awfm_candidates.c).  The reference has no
 * analogue (it stops at positions: ref src/AwFmParallelSearch.c:315-365).
 *
 * One routine, candidatesOfRead<THREADS, CAP>, does a read with a workgroup of THREADS threads and room for CAP kept hits:
 *
 *   check    awfm_hits_kernel.h's: a malformed read is reported and read no further.
 *   gather   awfm_hits_kernel.h's.  Kept hits are appended to LDS as (sequence, diagonal ^ 2^63) through one LDS atomic per wave
 *            and round; the counter runs on beyond CAP, so that it ends as the true number of kept hits.
 *   sort     bitonic, in LDS, over the next power of two (padding sorts last: no kept hit has sequence 0xFFFFFFFF).
 *   runs     a neighbour compare marks the heads; an inclusive max-scan gives every hit its head, and the last hit of a run
 *            leaves its own number at the head: votes, diagonal and span of a cluster are then read at its head.
 *   select   C rounds of a workgroup-wide arg-max over (votes, -head), each round below the winner before it.
 *   interval the smallest anchor and largest seedEnd of the at most 16 selected clusters come from a second pass over the same
 *            stretch (L2 hits): a kept hit belongs to the selected cluster whose (sequence, [diagonal, diagonal + span]) holds
 *            it.  Skipped when neither readBegins nor readEnds is asked for.  The sort so carries no payload: 14 bytes of LDS
 *            per kept hit.
 *
 * The two tiers of awfm_hits_kernel.h run it.  readCandidatesWaveKernel: CAP = kCandidatesWaveLimit; a read with more kept
 * hits, up to AWFM_CANDIDATES_MAX_HITS, goes onto the worklist (its gather has then only counted).  readCandidatesGroupKernel:
 * workgroups of kCandidatesGroupThreads with CAP = AWFM_CANDIDATES_MAX_HITS (58 KB of LDS: two workgroups per CU).  Reads beyond
 * that are overflowed: reported by the wave tier, never sorted.
 *
 * Vector loads and stores only; outputs are stored per read in whole runs of slots by the first C threads.
 */
#ifndef AWFM_CANDIDATES_KERNEL_H
#define AWFM_CANDIDATES_KERNEL_H

#include <type_traits>

#include "awfm_hits_kernel.h"

namespace {

constexpr unsigned kCandidatesWaveLimit = 256;    /* kept hits a wave sorts by itself: four per lane */
constexpr unsigned kCandidatesGroupLimit = 4096;  /* = AWFM_CANDIDATES_MAX_HITS */
constexpr unsigned kCandidatesWaveThreads = 64;   /* per workgroup of the wave tier: one wave */
constexpr unsigned kCandidatesGroupThreads = 512; /* per workgroup of the workgroup tier: eight hits per thread */
constexpr unsigned kCandidatesEntryBytes = 14;    /* LDS per kept hit: sequence 4, diagonal 8, head or last 2 */
constexpr unsigned kCandidatesWaveLdsBytes = 4608;   /* static LDS of the wave tier's kernel at the most (3584 + slots): 4.5 KB */
constexpr unsigned kCandidatesGroupLdsBytes = 59392; /* ... and of the workgroup tier's (57344 + slots): 58 KB */
constexpr unsigned kCandidatesSlots = 16;         /* = AWFM_CANDIDATES_MAX_SLOTS */

static_assert(kCandidatesGroupLimit == AWFM_CANDIDATES_MAX_HITS && kCandidatesSlots == AWFM_CANDIDATES_MAX_SLOTS, "include/awfm_gpu.h");
static_assert(kCandidatesGroupLimit <= 4096, "a head's number and 12 bits of votes share 32 bits; heads are stored in 16");

struct DevCandidateParams {
  AwFmCandidateInputs in;
  AwFmCandidateOutputs out;
  unsigned long long numReads;
  unsigned maxHitsPerSeed, band, minVotes, slots;
  unsigned waveLimit;          /* kept hits up to which the wave tier does a read itself (0: every read goes to the worklist) */
  unsigned long long *counter; /* dScratch: the worklist's length ... */
  unsigned *worklist;          /* ... and its numReads entries */
};

/* LDS of one workgroup */
template <unsigned CAP>
struct CandidatesLds {
  unsigned long long key[CAP];
  unsigned sequence[CAP];
  unsigned short aux[CAP]; /* the hit's head; at a head, once the runs are known: the run's last hit */
  unsigned long long kept; /* appended so far: the true number of kept hits in the end */
  unsigned long long selLow[kCandidatesSlots], selHigh[kCandidatesSlots];
  unsigned selSequence[kCandidatesSlots], selBegin[kCandidatesSlots], selEnd[kCandidatesSlots];
  unsigned best[kCandidatesSlots]; /* round j's winner: votes * 4096 + (4095 - head), 0: none */
  unsigned numCandidates;
};
static_assert(sizeof(CandidatesLds<kCandidatesWaveLimit>) <= kCandidatesWaveLdsBytes, "the wave tier's LDS");
static_assert(sizeof(CandidatesLds<kCandidatesGroupLimit>) <= kCandidatesGroupLdsBytes, "the workgroup tier's LDS");

/* The output pointers where they are stored through, not before (kernelArguments): the kernel's arguments are 26 words and
 * pointers, and the sort spills scalar registers when they are loaded ahead of the loop over the reads. */
typedef const __attribute__((address_space(4))) AwFmCandidateOutputs *KernelOutputs;
__device__ __forceinline__ KernelOutputs outputsOf() { return &kernelArguments<DevCandidateParams>()->out; }

/* stores read r's slots from `first` on as unused, by the first threads of the workgroup */
__device__ __forceinline__ void fillSlots(const DevCandidateParams &p, KernelOutputs out, unsigned long long r, unsigned first) {
  const unsigned j = threadIdx.x;
  if (j < first || j >= p.slots) return;
  const unsigned long long at = r * p.slots + j;
  if (out->sequences) out->sequences[at] = kHitsNone;
  if (out->diagonals) out->diagonals[at] = 0;
  if (out->votes) out->votes[at] = 0u;
  if (out->diagonalSpans) out->diagonalSpans[at] = 0u;
  if (out->readBegins) out->readBegins[at] = 0u;
  if (out->readEnds) out->readEnds[at] = 0u;
}

/* a read without candidates of its own: malformed, overflowed, or left to the other tier (then nothing is stored) */
__device__ __forceinline__ void reportUnsorted(const DevCandidateParams &p, unsigned long long r, unsigned keptHits) {
  const KernelOutputs out = outputsOf();
  fillSlots(p, out, r, 0u);
  if (threadIdx.x == 0u) {
    if (out->numCandidates) out->numCandidates[r] = 0u;
    if (out->keptHits) out->keptHits[r] = keptHits;
    if (out->numOverflowed) atomicAdd((unsigned long long *)out->numOverflowed, 1ull);
  }
}

/* Read r by the calling workgroup.  Returns true when the read has more than `limit` (<= CAP) but at most
 * AWFM_CANDIDATES_MAX_HITS kept hits: nothing was stored, the read is the other tier's.  Workgroup-uniform. */
template <unsigned THREADS, unsigned CAP>
__device__ bool candidatesOfRead(const DevCandidateParams &p, CandidatesLds<CAP> &s, unsigned long long r, unsigned limit) {
  constexpr unsigned kPer = CAP / THREADS; /* hits per thread once they are in LDS */
  static_assert(CAP % THREADS == 0 && (CAP & (CAP - 1u)) == 0, "a power of two, whole rounds");
  const unsigned tid = threadIdx.x;
  __syncthreads(); /* the LDS of the read before */
  if (tid == 0u) {
    s.kept = 0ull;
    s.numCandidates = 0u;
  }
  if (tid < kCandidatesSlots) {
    s.best[tid] = 0u;
    s.selBegin[tid] = 0xFFFFFFFFu;
    s.selEnd[tid] = 0u;
  }
  /* check */
  unsigned long long seedBegin, seedEnd;
  if (__syncthreads_or(readMalformed<THREADS>(p.in, r, seedBegin, seedEnd))) {
    reportUnsorted(p, r, kHitsMalformed);
    return false;
  }
  /* gather */
  unsigned long long low, high;
  wavePart<THREADS>(p.in, seedBegin, seedEnd, low, high);
  const unsigned lane = tid & 63u;
  visitHits(p, seedBegin, seedEnd, low, high, [&](bool keep, unsigned sequence, unsigned long long key, unsigned, unsigned) {
    const unsigned long long mask = __ballot(keep);
    if (mask == 0ull) return;
    const unsigned long long at = waveAppend(&s.kept, mask, __ffsll((long long)mask) - 1);
    if (keep && at < CAP) {
      s.sequence[at] = sequence;
      s.key[at] = key;
    }
  });
  __syncthreads();
  const unsigned long long kept = s.kept;
  if (kept > kCandidatesGroupLimit) {
    reportUnsorted(p, r, keptHitsWord(kept));
    return false;
  }
  if (kept > limit) return true;
  const unsigned n = (unsigned)kept;
  /* sort: by (sequence, key) */
  struct Hit {
    unsigned sequence;
    unsigned long long key;
  };
  sortLds<THREADS>(
      n, Hit{kHitsNone, ~0ull}, [&](unsigned i) { return Hit{s.sequence[i], s.key[i]}; },
      [&](unsigned i, const Hit &x) {
        s.sequence[i] = x.sequence;
        s.key[i] = x.key;
      },
      [](const Hit &x, const Hit &y) { return x.sequence != y.sequence ? x.sequence > y.sequence : x.key > y.key; });
  /* runs: thread tid has the hits tid, tid + THREADS, ... */
  unsigned heads = 0u, lasts = 0u; /* bit e: my hit e begins / ends a run */
#pragma unroll
  for (unsigned e = 0; e < kPer; e++) {
    const unsigned i = tid + e * THREADS;
    if (i < n) {
      const bool head = i == 0u || s.sequence[i] != s.sequence[i - 1u] || s.key[i] - s.key[i - 1u] > p.band;
      const bool last = i + 1u == n || s.sequence[i + 1u] != s.sequence[i] || s.key[i + 1u] - s.key[i] > p.band;
      heads |= (head ? 1u : 0u) << e;
      lasts |= (last ? 1u : 0u) << e;
      s.aux[i] = (unsigned short)(head ? i : 0u);
    }
  }
  __syncthreads();
  for (unsigned d = 1u; d < n; d <<= 1) { /* inclusive max-scan: the hit's head */
    unsigned short before[kPer];
#pragma unroll
    for (unsigned e = 0; e < kPer; e++) {
      const unsigned i = tid + e * THREADS;
      before[e] = i < n && i >= d ? s.aux[i - d] : (unsigned short)0;
    }
    __syncthreads();
#pragma unroll
    for (unsigned e = 0; e < kPer; e++) {
      const unsigned i = tid + e * THREADS;
      if (i < n && before[e] > s.aux[i]) s.aux[i] = before[e];
    }
    __syncthreads();
  }
  unsigned short headOf[kPer];
#pragma unroll
  for (unsigned e = 0; e < kPer; e++) {
    const unsigned i = tid + e * THREADS;
    headOf[e] = i < n ? s.aux[i] : (unsigned short)0;
  }
  __syncthreads();
#pragma unroll
  for (unsigned e = 0; e < kPer; e++)
    if ((lasts >> e) & 1u) s.aux[headOf[e]] = (unsigned short)(tid + e * THREADS);
  __syncthreads();
  /* select */
  unsigned packed[kPer]; /* votes * 4096 + (4095 - head) of the candidates among my hits: larger is better, none are equal */
  unsigned mine = 0u;
#pragma unroll
  for (unsigned e = 0; e < kPer; e++) {
    const unsigned i = tid + e * THREADS;
    packed[e] = 0u;
    if ((heads >> e) & 1u) {
      const unsigned votes = (unsigned)s.aux[i] - i + 1u;
      if (votes >= p.minVotes) {
        packed[e] = votes * 4096u + (4095u - i);
        mine++;
      }
    }
  }
  if (mine) atomicAdd(&s.numCandidates, mine);
  unsigned below = 0xFFFFFFFFu;
  for (unsigned j = 0; j < p.slots; j++) {
    unsigned best = 0u;
#pragma unroll
    for (unsigned e = 0; e < kPer; e++) best = packed[e] < below && packed[e] > best ? packed[e] : best;
#pragma unroll
    for (int offset = 32; offset > 0; offset >>= 1) {
      const unsigned other = (unsigned)__shfl_xor((int)best, offset, 64);
      best = other > best ? other : best;
    }
    if (lane == 0u && best) atomicMax(&s.best[j], best);
    __syncthreads();
    below = s.best[j];
    if (below == 0u) break; /* (uniform) */
  }
  __syncthreads();
  const unsigned numCandidates = s.numCandidates;
  const unsigned stored = numCandidates < p.slots ? numCandidates : p.slots;
  const KernelOutputs out = outputsOf();
  const bool intervals = out->readBegins || out->readEnds;
  if (tid < stored) {
    const unsigned i = 4095u - (s.best[tid] & 4095u), lastHit = s.aux[i];
    s.selSequence[tid] = s.sequence[i];
    s.selLow[tid] = s.key[i];
    s.selHigh[tid] = s.key[lastHit];
  }
  __syncthreads();
  if (intervals && stored != 0u) { /* the selected clusters' read intervals: the stretch once more */
    visitHits(p, seedBegin, seedEnd, low, high, [&](bool keep, unsigned sequence, unsigned long long key, unsigned anchor, unsigned end) {
      if (!keep) return;
      for (unsigned j = 0; j < stored; j++)
        if (sequence == s.selSequence[j] && key >= s.selLow[j] && key <= s.selHigh[j]) {
          atomicMin(&s.selBegin[j], anchor);
          atomicMax(&s.selEnd[j], end);
        }
    });
    __syncthreads();
  }
  if (tid < stored) {
    const unsigned long long at = r * p.slots + tid, span = s.selHigh[tid] - s.selLow[tid];
    if (out->sequences) out->sequences[at] = s.selSequence[tid];
    if (out->diagonals) out->diagonals[at] = (long long)(s.selLow[tid] ^ kHitsSign);
    if (out->votes) out->votes[at] = s.best[tid] >> 12;
    if (out->diagonalSpans) out->diagonalSpans[at] = span > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned)span;
    if (out->readBegins) out->readBegins[at] = s.selBegin[tid];
    if (out->readEnds) out->readEnds[at] = s.selEnd[tid];
  }
  fillSlots(p, out, r, stored);
  if (tid == 0u) {
    if (out->numCandidates) out->numCandidates[r] = numCandidates;
    if (out->keptHits) out->keptHits[r] = n;
  }
  return false;
}

/* the wave tier: what it cannot hold goes onto the worklist */
__global__ void __launch_bounds__(kCandidatesWaveThreads) readCandidatesWaveKernel(const DevCandidateParams p) {
  __shared__ CandidatesLds<kCandidatesWaveLimit> s;
  waveTier(p, blockIdx.x, gridDim.x, [&](unsigned long long r) { return candidatesOfRead<kCandidatesWaveThreads, kCandidatesWaveLimit>(p, s, r, p.waveLimit); });
}

/* the workgroup tier */
__global__ void __launch_bounds__(kCandidatesGroupThreads) readCandidatesGroupKernel(const DevCandidateParams p) {
  __shared__ CandidatesLds<kCandidatesGroupLimit> s;
  groupTier(p, blockIdx.x, gridDim.x, [&](unsigned long long r) {
    return candidatesOfRead<kCandidatesGroupThreads, kCandidatesGroupLimit>(p, s, r, kCandidatesGroupLimit);
  });
}

/* kernelArguments() reads the argument segment as a DevCandidateParams: right only while that struct is the one argument of both
 * kernels, by value, hence at offset 0.  A change of either signature stops the build here. */
static_assert(std::is_same<decltype(&readCandidatesWaveKernel), void (*)(DevCandidateParams)>::value &&
                  std::is_same<decltype(&readCandidatesGroupKernel), void (*)(DevCandidateParams)>::value,
              "kernelArguments() assumes DevCandidateParams is the kernels' only argument");

}  // namespace

#endif
