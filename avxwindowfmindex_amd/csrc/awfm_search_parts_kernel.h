/*
 * awfm_search_parts_kernel.h -- what the hits-only search kernels share (awfm_ordered_kernel.h, awfm_mixed_lookup_kernel.h,
 * awfm_amino_lookup_kernel.h) and, of the scan, the kernels of awfm_gpu_locate.hip and awfm_gpu_ordered.hip.  One definition each;
 * the kernels keep their LDS slots, their loops over trips, rounds and passes, their gates and what they measured.
 *
 *   letters    decodeWord / decodeWordAny / decodeKmer: ASCII nucleotides to 2-bit codes; alignedFour / decodeFour: the FOUR
 *              consecutive k-mers of a thread from 16-byte loads.
 *   share      shareRange: the k-mers of the batch that a workgroup of a share-wise launch strides over.
 *   entry      deepEntryAlive: does an entry of the deeper table leave its k-mer anything to search.
 *   steps      hitsStep: the next step of a hits-only k-mer -- two characters by one pair step, or one by a single step.
 *   hit list   HitList: the per-wave buffers behind SparseOut::count (append, flush, finish).
 *   scan       blockInclusiveScan: one value per thread, over the workgroup.
 *
 * Vector loads and stores only.
 */
#ifndef AWFM_SEARCH_PARTS_KERNEL_H
#define AWFM_SEARCH_PARTS_KERNEL_H

#include "awfm_device.h"
#include "awfm_pair.h"

namespace {

/* ------------------------------------------------------------------ letters */

/* 4 characters -> 4 two-bit codes (first character in bits 7..6) and 4 "not a,c,g,t,u" flags (bit i = character i);
 * same SWAR decode as the window decode of searchKernel */
__device__ __forceinline__ void decodeWord(unsigned word, unsigned &packed, unsigned &badBits) {
  unsigned t = (word >> 1) & 0x03030303u;
  t ^= (t >> 1) & 0x01010101u;
  const unsigned b0 = t & 0x01010101u, b1 = (t >> 1) & 0x01010101u, b01 = b0 & b1;
  const unsigned expect = 0x61616161u + (b0 << 1) + b1 * 6u + b01 * 11u; /* 'a','c','g','t' */
  unsigned diff = ((word | 0x20202020u) ^ expect) & ~b01;
  diff |= diff >> 4;
  diff |= diff >> 2;
  diff |= diff >> 1;
  diff &= 0x01010101u;
  badBits = (diff & 1u) | ((diff >> 7) & 2u) | ((diff >> 14) & 4u) | ((diff >> 21) & 8u);
  packed = ((t & 3u) << 6) | ((t >> 4) & 0x30u) | ((t >> 14) & 0x0Cu) | (t >> 24);
}

/* The same for a kernel that only asks whether ANY character of a k-mer is not a,c,g,t,u: the expected letters come from
 * one byte permute ('a','c','g','t' selected by the codes), and the differences of the characters that count
 * (`countMask`: 0xFF per character of the k-mer in this word) are OR-ed into `diffs` as they are.  decodeWord: 35 VALU
 * instructions per word, this: 19 -- encodeCodes4Kernel was bound by its VALU instructions (94 % of its cycles), not by its
 * 2.9 GB. */
__device__ __forceinline__ void decodeWordAny(unsigned word, unsigned countMask, unsigned &packed, unsigned &diffs) {
  unsigned t = (word >> 1) & 0x03030303u;
  t ^= (t >> 1) & 0x01010101u;
  const unsigned b01 = t & (t >> 1) & 0x01010101u;                   /* code 3: 't' or 'u' (they differ in bit 0) */
  const unsigned expect = __builtin_amdgcn_perm(0u, 0x74676361u, t); /* byte i = "acgt"[code i] */
  diffs |= ((word | 0x20202020u) ^ expect) & ~b01 & countMask;
  packed = ((t & 3u) << 6) | ((t >> 4) & 0x30u) | ((t >> 14) & 0x0Cu) | (t >> 24);
}

/* 2-bit codes (last character in bits 1..0) and ambiguity mask (bit i = character i is not a,c,g,t,u) of the `len`
 * (1..32) ASCII characters at chars + start: the aligned dwords that hold them, a dword only read when it contains one */
__device__ __forceinline__ void decodeKmer(const unsigned char *__restrict__ chars, unsigned long long start, unsigned len,
                                           unsigned long long &codes, unsigned &bad) {
  const unsigned long long at = (unsigned long long)chars + start;
  /* (an integer turned pointer is a generic one, read by FLAT loads: say that it is global memory) */
  typedef const unsigned __attribute__((address_space(1))) *GlobalWords;
  const GlobalWords first = (GlobalWords)(at & ~3ull);
  const unsigned shift = (unsigned)at & 3u;
  const unsigned numDwords = (shift + len + 3u) >> 2;
  unsigned dw[9];
#pragma unroll
  for (int j = 0; j < 9; j++) dw[j] = (unsigned)j < numDwords ? first[j] : 0u;
  codes = 0;
  bad = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    unsigned packed = 0, badBits = 0;
    if (4u * j < len) decodeWord(__builtin_amdgcn_alignbyte(dw[j + 1], dw[j], shift), packed, badBits);
    codes = (codes << 8) | packed;
    bad |= badBits << (4 * j);
  }
  codes >>= 2u * (32u - len); /* character 0 was in bits 63..62: now the last character is in bits 1..0 */
  bad &= len >= 32u ? ~0u : ((1u << len) - 1u);
}

/* A thread takes FOUR consecutive k-mers of a length known at compile time -- 4 K bytes, i.e. K whole dwords wherever the
 * batch starts -- with 16-byte loads and brings them to dword alignment once (`shift`: the misalignment of the batch, the
 * same for every thread): K / 4 + 1 load instructions per four k-mers instead of K / 4 + 2 per k-mer at a K-byte stride,
 * which is what bounds a kernel that decodes, not the bytes.  The last k-mers of a batch, whose loads would run past its end,
 * go one by one: fourAligned says which way it is. */
typedef unsigned Dwords4 __attribute__((ext_vector_type(4), aligned(4))); /* a 16-byte load at dword alignment */
template <unsigned K>
__device__ __forceinline__ bool fourAligned(unsigned long long t, unsigned long long numQueries) {
  constexpr unsigned kLoads = (K + 1u + 3u) / 4u; /* 16-byte loads that cover K + 1 dwords */
  return t * K + 16ull * kLoads <= numQueries * K; /* the 16-byte loads from the aligned-down start stay inside the batch */
}
/* al[0 .. K): the 4 K bytes of the k-mers t .. t + 3 at dword alignment (fourAligned) */
template <unsigned K>
__device__ __forceinline__ void alignedFour(const unsigned char *__restrict__ chars, unsigned shift, unsigned long long t, unsigned (&al)[K + 1u]) {
  constexpr unsigned kLoads = (K + 1u + 3u) / 4u;
  typedef const Dwords4 __attribute__((address_space(1))) *GlobalDwords4;
  const GlobalDwords4 from = (GlobalDwords4)(((unsigned long long)chars + t * K) & ~3ull);
  unsigned dw[kLoads * 4u + 1u];
#pragma unroll
  for (unsigned j = 0; j < kLoads; j++) {
    const Dwords4 q = from[j];
    dw[4u * j] = q.x;
    dw[4u * j + 1u] = q.y;
    dw[4u * j + 2u] = q.z;
    dw[4u * j + 3u] = q.w;
  }
  dw[kLoads * 4u] = 0u;
#pragma unroll
  for (unsigned j = 0; j < K; j++) al[j] = __builtin_amdgcn_alignbyte(dw[j + 1u], dw[j], shift);
  al[K] = 0u;
}
/* the nucleotide k-mers t .. t + 3 as codes (decodeKmer's) and "has a character that is not a,c,g,t,u" (bad != 0), taken
 * apart at compile-time offsets; a k-mer past the end of the batch: codes 0, bad 0 */
template <unsigned K>
__device__ __forceinline__ void decodeFour(const unsigned char *__restrict__ chars, unsigned shift, unsigned long long t,
                                           unsigned long long numQueries, unsigned long long (&codes)[4], unsigned (&bad)[4]) {
  if (fourAligned<K>(t, numQueries)) {
    unsigned al[K + 1u];
    alignedFour<K>(chars, shift, t, al);
#pragma unroll
    for (unsigned i = 0; i < 4u; i++) {
      constexpr unsigned kWords = (K + 3u) / 4u; /* groups of four characters */
      const unsigned at = i * K; /* byte offset of k-mer i: compile time after unrolling */
      unsigned long long c = 0;
      unsigned b = 0;
#pragma unroll
      for (unsigned w = 0; w < 8u; w++) {
        unsigned packed = 0;
        if (w < kWords) {
          const unsigned lo = al[(at >> 2) + w], hi = (at >> 2) + w + 1u <= K ? al[(at >> 2) + w + 1u] : 0u;
          const unsigned inKmer = K - 4u * w >= 4u ? 4u : K - 4u * w; /* characters of the k-mer in this word */
          decodeWordAny(__builtin_amdgcn_alignbyte(hi, lo, at & 3u), inKmer >= 4u ? ~0u : (1u << (8u * inKmer)) - 1u, packed, b);
        }
        c = (c << 8) | packed;
      }
      codes[i] = c >> (2u * (32u - K));
      bad[i] = b;
    }
  } else {
#pragma unroll
    for (unsigned i = 0; i < 4u; i++) {
      codes[i] = 0;
      bad[i] = 0;
      if (t + i < numQueries) decodeKmer(chars, (t + i) * K, K, codes[i], bad[i]);
    }
  }
}

/* ------------------------------------------------------------------ share */

constexpr unsigned kPartitionThreads = 1024, kPartitionItems = 16, kPartitionTile = kPartitionThreads * kPartitionItems;
/* The batch is cut into 8 SHARES of whole tiles, one per XCD (workgroup b works on share b % 8, the XCD it runs on under
 * round-robin dispatch: for speed only), and every bucket's place in the order into 8 sub-runs, share by share.  The
 * workgroups that append to a sub-run are then on ONE XCD: its L2 sees all the 64-byte runs that make up a line and writes
 * the line once, and the cursor it bumps is not shared with the other seven.  (One run area per bucket for the whole chip:
 * 1.2 GB written for 0.8 GB of records.) */
constexpr unsigned kShares = 8;
__host__ __device__ inline unsigned long long shareSize(unsigned long long numQueries) {
  const unsigned long long perShare = (numQueries + kShares - 1ull) / kShares;
  return (perShare + kPartitionTile - 1ull) / kPartitionTile * kPartitionTile;
}
/* a workgroup's share of the batch: workgroup localBlock of the localGrid that work on the k-mers [first, last) of `share` */
struct ShareRange {
  unsigned share, localBlock, localGrid;
  unsigned long long first, last; /* first: a multiple of the tile, hence of 4 */
};
__device__ __forceinline__ ShareRange shareRange(unsigned long long numQueries) {
  ShareRange r;
  r.share = blockIdx.x % kShares;
  r.localBlock = blockIdx.x / kShares;
  r.localGrid = gridDim.x / kShares;
  const unsigned long long size = shareSize(numQueries);
  r.first = size * r.share;
  r.last = r.first + size < numQueries ? r.first + size : numQueries;
  return r;
}

/* ------------------------------------------------------------------ entry */

/* Does entry `e` of the deeper table (8-byte entries, DevIndex::deepNarrow 1 or 2; lengthBits: deepLengthBits) keep a k-mer
 * alive: its range holds something, and -- useNext: the table has its next-step bits and they are in use -- so will the range
 * after the pair step of the two characters beyond the table (`beyond`: the k-mer's codes from those two on) */
__device__ __forceinline__ bool deepEntryAlive(uint2 e, unsigned lengthBits, bool useNext, unsigned long long beyond) {
  return (e.y & lengthBits) != 0u && (!useNext || ((e.y >> (16u + ((unsigned)beyond & 15u))) & 1u) != 0u);
}

/* ------------------------------------------------------------------ steps */

/* The next step of a hits-only k-mer by the G lanes of its group: rem = the codes of the characters to go (the next one in
 * bits 1..0), pos = their number - 1, {sp, ep} not empty.
 *   PAIR (G = 4, pos >= 1; the caller's flag, uniform): two characters per block read through the pair image; a block with
 *     an ambiguity letter or the sentinel is flagged, and both go letter by letter through the one-letter image.  Only hits
 *     are reported, so it does not matter at which of the two steps a range without hits became empty.
 *   otherwise (pos >= 0): one character through the one-letter image.
 * The callers' loops decide which: an odd character is taken alone and last -- few k-mers are still alive then, and the first
 * step from the deeper table is the pair step its next-step bits speak about.  (The instrumented loops -- orderedSearchKernel's,
 * whose TOUCH twin shares its text, and mixedLookupTallyKernel's -- mark lines between these calls and keep their own copy:
 * through this function the pair variants of the first lose registers, two to four more spilled, and the second a wave per SIMD.) */
template <int G, bool NARROW>
__device__ __forceinline__ void hitsStep(const bool PAIR, const DevIndex &ix, const unsigned long long *sC, const unsigned long long *sSuper,
                                         const unsigned *sMask, const unsigned long long *sPairC, const unsigned *sPairSuper,
                                         unsigned gl, unsigned firstSlice, unsigned long long &rem, int &pos,
                                         typename PositionType<NARROW>::type &sp, typename PositionType<NARROW>::type &ep) {
  if (PAIR) {
    const unsigned c2 = (unsigned)rem & 3u, c1 = (unsigned)(rem >> 2) & 3u;
    if (pairSearchStep<NARROW>(ix, sPairC, sPairSuper, sMask, gl, c1 * 4u + c2, sp, ep) == kPairFlagged) {
      nucFastStep<G, NARROW>(ix, sC, sSuper, sMask, firstSlice, c2, sp, ep);
      if (sp <= ep) nucFastStep<G, NARROW>(ix, sC, sSuper, sMask, firstSlice, c1, sp, ep);
    }
    pos -= 2;
    rem >>= 4;
  } else {
    nucFastStep<G, NARROW>(ix, sC, sSuper, sMask, firstSlice, (unsigned)rem & 3u, sp, ep);
    pos--;
    rem >>= 2;
  }
}

/* ------------------------------------------------------------------ hit list */

/* The list of hits (SparseOut::count) of a kernel whose waves find their hits a few at a time: a wave collects them in LDS
 * and appends them kHitBuffer at a time, and what the waves of a workgroup still hold when they are done goes out in ONE
 * reservation, made by the wave that finishes last.  (One returning atomic per wave round with a hit is 7 * 10^4 atomics on
 * one word for 10^8 random 21-mers, and a word takes 88 per microsecond: 0.8 ms.  The waves of a grid end together, and 7168
 * of them each taking a returning atomic on the list's counter were a tail of 60-80 us on a kernel that searched 5 * 10^5
 * k-mers.)  Entries beyond SparseOut::cap are counted, not stored.
 * `__shared__ HitList<WAVES> sHits;` beside a word `wavesDone` of LDS that is zeroed before the workgroup's first barrier (a
 * variable of its own: inside the struct it would pad the struct, and the kernels' LDS, by 8 bytes); EXISTS = false: the
 * variant of a kernel that has no list keeps one-element arrays.  The wave's fill is the caller's (wave-uniform, 0 at
 * first), w = its wave in the workgroup (uniform), lane = its lane. */
constexpr unsigned kHitBuffer = 32;
template <unsigned WAVES, bool EXISTS = true>
struct HitList {
  static constexpr unsigned kWaves = EXISTS ? WAVES : 1u, kBuffer = EXISTS ? kHitBuffer : 1u;
  unsigned long long ranges[kWaves][kBuffer][2];
  unsigned kmers[kWaves][kBuffer];
  unsigned left[kWaves];

  /* wave-uniform: the wave's collected hits go to the list, one reservation for all of them */
  __device__ __forceinline__ void flush(const SparseOut &sparse, unsigned w, unsigned lane, unsigned &fill) {
    if (fill != 0u) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      unsigned listBase = 0;
      if (lane == 0) listBase = atomicAdd(sparse.count, fill);
      listBase = (unsigned)__builtin_amdgcn_readfirstlane((int)listBase);
      if (lane < fill && listBase + lane < sparse.cap) {
        sparse.kmers[listBase + lane] = kmers[w][lane];
        sparse.ranges[listBase + lane] = make_ulonglong2(ranges[w][lane][0], ranges[w][lane][1]);
      }
      __builtin_amdgcn_wave_barrier();
      fill = 0;
    }
  }
  /* wave-uniform call; hit: in one lane of each group of G that has one, k-mer `index` with the range {sp, ep}.  There is room:
   * the buffer is emptied whenever the hits of another call -- 64 / G at most -- might not fit. */
  template <int G>
  __device__ __forceinline__ void append(const SparseOut &sparse, unsigned w, unsigned lane, unsigned &fill, bool hit, unsigned index,
                                         unsigned long long sp, unsigned long long ep) {
    const unsigned long long hitMask = __ballot(hit);
    if (hitMask != 0ull) { /* wave-uniform */
      const unsigned hits = (unsigned)__builtin_amdgcn_readfirstlane((int)__popcll(hitMask));
      if (hit) {
        const unsigned at = fill + (unsigned)__popcll(hitMask & ((1ull << lane) - 1ull));
        kmers[w][at] = index;
        ranges[w][at][0] = sp;
        ranges[w][at][1] = ep;
      }
      fill = (unsigned)__builtin_amdgcn_readfirstlane((int)(fill + hits));
    }
    if (fill + 64u / G > kBuffer) flush(sparse, w, lane, fill);
  }
  /* every wave, once, when it is done: the waves' leftovers in one reservation */
  __device__ __forceinline__ void finish(const SparseOut &sparse, unsigned w, unsigned lane, unsigned fill, unsigned &wavesDone) {
    if (lane == 0) left[w] = fill;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    unsigned arrived = 0;
    if (lane == 0) arrived = atomicAdd(&wavesDone, 1u);
    arrived = (unsigned)__builtin_amdgcn_readfirstlane((int)arrived);
    if (arrived == kWaves - 1u) { /* wave-uniform: every wave's leftovers are in LDS */
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      unsigned total = 0;
      for (unsigned v = 0; v < kWaves; v++) total += left[v];
      if (total != 0u) {
        unsigned listBase = 0;
        if (lane == 0) listBase = atomicAdd(sparse.count, total);
        listBase = (unsigned)__builtin_amdgcn_readfirstlane((int)listBase);
        unsigned before = 0;
        for (unsigned v = 0; v < kWaves; v++) {
          const unsigned n = left[v]; /* at most kHitBuffer <= 64 */
          if (lane < n && listBase + before + lane < sparse.cap) {
            sparse.kmers[listBase + before + lane] = kmers[v][lane];
            sparse.ranges[listBase + before + lane] = make_ulonglong2(ranges[v][lane][0], ranges[v][lane][1]);
          }
          before += n;
        }
      }
    }
  }
};

/* ------------------------------------------------------------------ scan */

/* Inclusive scan of one value per thread over a workgroup of whole waves: the sum of the values of the threads up to and
 * including this one.  sWave: a word per wave, which holds the waves' totals afterwards.  Every thread calls it (a barrier
 * inside), and a barrier stands between two calls that use the same sWave. */
template <class T>
__device__ __forceinline__ T blockInclusiveScan(T value, T *sWave) {
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  T incl = value;
  for (int d = 1; d < 64; d <<= 1) {
    const T up = __shfl_up(incl, d, 64);
    if (lane >= (unsigned)d) incl += up;
  }
  if (lane == 63u) sWave[wave] = incl;
  __syncthreads();
  for (unsigned w = 0; w < wave; w++) incl += sWave[w];
  return incl;
}

}  // namespace

#endif
