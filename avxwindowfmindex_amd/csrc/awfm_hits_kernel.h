/*
 * awfm_hits_kernel.h -- what the kernels of "candidate loci" and "read chains" share (awfm_candidates_kernel.h,
 * awfm_chains_kernel.h): the device's definition of a read's KEPT HITS (include/awfm_gpu.h, "candidate loci") and the two tiers
 * that both units run -- and what their launchers share (awfm_gpu_candidates.hip, awfm_gpu_chains.hip).  The host's definition
 * of the same things is awfm_hits.h.
 *
 *   check    readMalformed: the read's seed range and the hit range of each of its seeds against the arrays' sizes, before
 *            anything is read through them.
 *   gather   a read's hits are ONE stretch of positions / sequenceNumbers (its seeds are contiguous, hitOffsets is CSR), so each
 *            wave streams a contiguous part of it (wavePart), 64 hits per round (visitHits); a hit finds its seed by a binary
 *            search over the read's few hit offsets (cache hits), and a wave that stands wholly inside a dropped seed jumps to
 *            that seed's end.  What a unit keeps of a round goes to LDS through one LDS atomic per wave (waveAppend).
 *   sort     sortLds: bitonic, in LDS, over the next power of two; the unit says what an entry is and how two compare.
 *   tiers    waveTier: one wave per read (workgroups of one wave, a persistent grid-stride loop over the reads); a read that is
 *            the other tier's is appended to a worklist by one lane.  groupTier: a fixed grid that reads the worklist's length
 *            on the device and gives each such read a workgroup.  launchTiers zeroes the length and launches both.
 *
 * A unit's parameter struct P has `in`, `maxHitsPerSeed`, `numReads`, `waveLimit`, `counter` and `worklist`.  Vector loads and
 * stores only.
 */
#ifndef AWFM_HITS_KERNEL_H
#define AWFM_HITS_KERNEL_H

#include <cstring>
#include <string>

#include "awfm_device.h"

namespace {

constexpr unsigned kHitsNone = 0xFFFFFFFFu;          /* = AWFM_CANDIDATES_NONE: the sequence of an illegal hit, an unused slot */
constexpr unsigned long long kHitsSign = 1ull << 63; /* key = diagonal ^ this: unsigned order = signed order */
constexpr unsigned kHitsMalformed = 0xFFFFFFFFu, kHitsSaturated = 0xFFFFFFFEu; /* keptHits words */
constexpr uint64_t kCounterBytes = 16; /* dScratch: the worklist's length, ahead of the worklist's numReads entries */

/* Calls visit(keep, sequence, key, anchor, end) for every hit of the stretch [hitLow, hitHigh) of a well-formed read, 64 per
 * round and wave, with keep = the hit is a kept hit; all 64 lanes make every call (visit may ballot). */
template <typename P, typename Visit>
__device__ __forceinline__ void visitHits(const P &p, unsigned long long seedBegin, unsigned long long seedEnd, unsigned long long hitLow,
                                          unsigned long long hitHigh, Visit visit) {
  const AwFmCandidateInputs &in = p.in;
  const unsigned lane = threadIdx.x & 63u;
  unsigned long long base = hitLow;
  while (base < hitHigh) { /* wave-uniform */
    const unsigned long long h = base + lane;
    const bool inside = h < hitHigh;
    const unsigned long long hh = inside ? h : base;
    unsigned long long lo = seedBegin, hi = seedEnd; /* the last seed whose hits begin at or before hh: hitOffsets[seedBegin] <= hh */
    while (hi - lo > 1u) {
      const unsigned long long mid = lo + ((hi - lo) >> 1);
      const bool before = in.hitOffsets[mid] <= hh;
      lo = before ? mid : lo;
      hi = before ? hi : mid;
    }
    const unsigned long long seedHitBegin = in.hitOffsets[lo], seedHitEnd = in.hitOffsets[lo + 1u];
    const unsigned length = in.seedLengths ? in.seedLengths[lo] : in.fixedLength, end = in.seedEnds[lo];
    const bool seedKept = length <= end && (p.maxHitsPerSeed == 0u || seedHitEnd - seedHitBegin <= p.maxHitsPerSeed);
    /* lane 0 stands at `base`: when its seed is dropped and holds the whole round, the wave goes on behind that seed */
    const unsigned long long firstEnd = (unsigned long long)__shfl((long long)seedHitEnd, 0, 64);
    if (!__shfl((int)seedKept, 0, 64) && firstEnd - base >= 64u) {
      base = firstEnd < hitHigh ? firstEnd : hitHigh;
      continue;
    }
    bool keep = inside && seedKept;
    unsigned sequence = 0;
    if (keep && in.sequenceNumbers) {
      sequence = in.sequenceNumbers[h];
      keep = sequence != kHitsNone;
    }
    const unsigned anchor = end - length;
    const unsigned long long key = keep ? (in.positions[h] - anchor) ^ kHitsSign : 0ull;
    visit(keep, sequence, key, anchor, end);
    base += 64u;
  }
}

/* the part [low, high) of the read's stretch of hits that this wave streams: the stretch in equal contiguous parts, one per wave */
template <unsigned THREADS>
__device__ __forceinline__ void wavePart(const AwFmCandidateInputs &in, unsigned long long seedBegin, unsigned long long seedEnd,
                                         unsigned long long &low, unsigned long long &high) {
  constexpr unsigned kWaves = THREADS / 64u;
  const unsigned wave = threadIdx.x >> 6;
  const unsigned long long hitBegin = seedBegin < seedEnd ? in.hitOffsets[seedBegin] : 0ull;
  const unsigned long long hitEnd = seedBegin < seedEnd ? in.hitOffsets[seedEnd] : 0ull;
  const unsigned long long part = (hitEnd - hitBegin + kWaves - 1u) / kWaves;
  low = hitBegin + wave * part;
  low = low < hitEnd ? low : hitEnd;
  high = hitEnd - low < part ? hitEnd : low + part;
}

/* Read r's seeds [seedBegin, seedEnd), and what this thread of THREADS sees of "the read is malformed": the caller ORs it over
 * the workgroup.  Nothing is read through an offset that was not compared with its array's size first. */
template <unsigned THREADS>
__device__ __forceinline__ bool readMalformed(const AwFmCandidateInputs &in, unsigned long long r, unsigned long long &seedBegin,
                                              unsigned long long &seedEnd) {
  seedBegin = in.readSeedOffsets[r];
  seedEnd = in.readSeedOffsets[r + 1u];
  bool malformed = seedBegin > seedEnd || seedEnd > in.numSeeds || seedEnd - seedBegin >= (1ull << 32);
  if (!malformed)
    for (unsigned long long q = seedBegin + threadIdx.x; q < seedEnd; q += THREADS)
      malformed |= in.hitOffsets[q] > in.hitOffsets[q + 1u] || in.hitOffsets[q + 1u] > in.numHits;
  return malformed;
}

/* the keptHits word of a well-formed read with that many kept hits */
__device__ __forceinline__ unsigned keptHitsWord(unsigned long long kept) { return kept > kHitsSaturated ? kHitsSaturated : (unsigned)kept; }

/* The places of a round's entries, by all 64 lanes: lane `leader` adds the number of lanes in `mask` to *counter (LDS) once, and
 * every lane gets what the counter held plus the lanes of mask below it -- its own entry's place when it is one of mask. */
template <typename T>
__device__ __forceinline__ T waveAppend(T *counter, unsigned long long mask, int leader) {
  const unsigned lane = threadIdx.x & 63u;
  T at = 0;
  if ((int)lane == leader && mask != 0ull) at = atomicAdd(counter, (T)__popcll(mask));
  return __shfl(at, leader, 64) + (T)__popcll(mask & ((1ull << lane) - 1ull));
}

/* The n entries a workgroup of THREADS has in LDS, sorted by a bitonic network over the next power of two.  load(i) gives the
 * Entry at position i, store(i, x) puts x there, greater(x, y) says whether x sorts behind y, `last` sorts behind every entry
 * (the padding).  An entry is loaded once per compare: the units' entries are two arrays wide. */
template <unsigned THREADS, typename Entry, typename Load, typename Store, typename Greater>
__device__ __forceinline__ void sortLds(unsigned n, const Entry last, Load load, Store store, Greater greater) {
  const unsigned tid = threadIdx.x;
  unsigned padded = 2u;
  while (padded < n) padded <<= 1;
  for (unsigned i = n + tid; i < padded; i += THREADS) store(i, last);
  __syncthreads();
  if (n > 1u)
    for (unsigned k = 2u; k <= padded; k <<= 1)
      for (unsigned j = k >> 1; j != 0u; j >>= 1) {
        for (unsigned t = tid; t < (padded >> 1); t += THREADS) {
          const unsigned a = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), b = a | j;
          const Entry x = load(a), y = load(b);
          if (greater(x, y) == ((a & k) == 0u)) {
            store(a, y);
            store(b, x);
          }
        }
        __syncthreads();
      }
}

/* The kernel's parameters where they are needed, not before: a unit's arguments are dozens of words and pointers, and the
 * compiler would otherwise load all of them ahead of the loop over the reads and spill scalar registers in the sort or the
 * recurrence.  They are read from the kernel's argument segment, of which P is the one and only entry in both kernels of a unit
 * (a static_assert on their signatures at the end of the unit's header holds that); the empty statement only hides where the
 * pointer comes from, so that the loads stay behind it. */
template <typename P>
__device__ __forceinline__ const __attribute__((address_space(4))) P *kernelArguments() {
  auto params = (const __attribute__((address_space(4))) P *)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(params));
  return params;
}

/* The wave tier's loop.  doRead(r) does read r with the calling workgroup and returns true (workgroup-uniform) when it stored
 * nothing because the read is the other tier's: then it goes onto the worklist.  block, blocks: the kernel's blockIdx.x and
 * gridDim.x, read by the kernel itself -- read in here, the compiler fetches the workgroup's size anew for every read. */
template <typename P, typename DoRead>
__device__ __forceinline__ void waveTier(const P &p, const unsigned block, const unsigned blocks, DoRead doRead) {
  for (unsigned long long r = block; r < p.numReads; r += blocks)
    if (doRead(r) && threadIdx.x == 0u)
      p.worklist[atomicAdd(p.counter, 1ull)] = (unsigned)r; /* (at most one entry per read: numReads entries hold them) */
}

/* the workgroup tier's loop: the reads of the worklist, whose length is read here */
template <typename P, typename DoRead>
__device__ __forceinline__ void groupTier(const P &p, const unsigned block, const unsigned blocks, DoRead doRead) {
  const unsigned long long have = *p.counter, listed = have < p.numReads ? have : p.numReads;
  for (unsigned long long w = block; w < listed; w += blocks) {
    const unsigned long long r = p.worklist[w];
    if (r < p.numReads) (void)doRead(r);
  }
}

/* ---- the launchers ---- */

/* What both calls refuse after "null image" and numReads == 0, in this order, with the call's name before the text: a null
 * among the inputs (others: the call's own pointers, false when one of them is null), seeds with neither lengths nor a fixed
 * length, more than 2^32 - 1 reads or a slot count outside 1 .. 16.  AwFmSuccess: nothing is refused */
inline enum AwFmReturnCode hitsArgumentsRefused(const char *name, const struct AwFmCandidateInputs *dIn, const bool others,
                                                const uint64_t numReads, const uint32_t maxCandidates) {
  const auto refuse = [name](const char *what, enum AwFmReturnCode rc) {
    setError((std::string(name) + ": " + what).c_str());
    return rc;
  };
  if (!dIn || !others || !dIn->readSeedOffsets || !dIn->seedEnds || !dIn->hitOffsets || !dIn->positions)
    return refuse("null argument", AwFmNullPtrError);
  if (!dIn->seedLengths && dIn->fixedLength == 0) return refuse("the seeds need their lengths or a fixed length", AwFmNullPtrError);
  if (numReads >= (1ull << 32) || maxCandidates < 1 || maxCandidates > AWFM_CANDIDATES_MAX_SLOTS)
    return refuse("read numbers are 32-bit, and a read has 1 to 16 slots", AwFmIllegalPositionError);
  return AwFmSuccess;
}

/* the bytes of dScratch for numReads reads: the worklist's length and one entry per read */
inline uint64_t hitsScratchBytes(uint64_t numReads) { return kCounterBytes + alignUp(numReads * 4u, 16); }

/* Enqueues a unit's two tiers on `stream` with p, of which everything but the tiers' own fields is filled in.  The wave tier
 * does reads of up to waveLimit entries itself; $AWFM_GPU_DIAG `tierKey`=group (tests) sends every read with an entry through the
 * workgroup tier, `wave` names the default, in which every read that fits the wave tier already takes it.  Persistent grids: 16
 * waves per CU of the wave tier, the two workgroups per CU that the workgroup tier's LDS leaves.  groupDynamicLds != 0: the
 * workgroup tier's LDS is dynamic and beyond what a kernel gets without asking.  The limit belongs to the kernel ON A DEVICE: it
 * is set under the guard at every call (a host-side table write), not once per process, which would leave every device but the
 * first call's without it */
template <typename P>
inline enum AwFmReturnCode launchTiers(const AwFmGpuIndex *g, P &p, const char *tierKey, unsigned waveLimit, void (*waveKernel)(P),
                                       unsigned waveThreads, void (*groupKernel)(P), unsigned groupThreads, unsigned groupDynamicLds,
                                       void *dScratch, void *stream) {
  DeviceGuard guard(g->device);
  p.waveLimit = waveLimit;
  if (const char *env = awfmGpuDiag(tierKey)) {
    if (!strcmp(env, "group")) p.waveLimit = 0;
  }
  p.counter = (unsigned long long *)dScratch;
  p.worklist = (unsigned *)((uint8_t *)dScratch + kCounterBytes);
  hipStream_t s = (hipStream_t)stream;
  if (groupDynamicLds != 0u)
    AWFM_HIP_TRY(hipFuncSetAttribute((const void *)groupKernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)groupDynamicLds),
                 AwFmGeneralFailure);
  AWFM_HIP_TRY(hipMemsetAsync(dScratch, 0, kCounterBytes, s), AwFmGeneralFailure);
  const uint64_t numReads = p.numReads, waveBlocks = (uint64_t)g->numCUs * 16u, groupBlocks = (uint64_t)g->numCUs * 2u;
  hipLaunchKernelGGL(waveKernel, dim3((unsigned)(numReads < waveBlocks ? numReads : waveBlocks)), dim3(waveThreads), 0, s, p);
  AWFM_HIP_TRY(hipGetLastError(), AwFmGeneralFailure);
  hipLaunchKernelGGL(groupKernel, dim3((unsigned)(numReads < groupBlocks ? numReads : groupBlocks)), dim3(groupThreads), groupDynamicLds, s,
                     p);
  AWFM_HIP_TRY(hipGetLastError(), AwFmGeneralFailure);
  return AwFmSuccess;
}

}  // namespace

#endif
