/*
 * awfm_strings_kernel.h -- stringLengthsKernel<WIDE> and stringWriteKernel<WIDE>, the kernels of "alignment strings"
 * (include/awfm_gpu.h).  The definition is the header's; the host twin and checker is awfm_strings.c.
 *
 * LENGTHS.  A THREAD takes a read: the work of a read is a sequential walk over its row of runs -- 10.9 of 32 words on the
 * measured batch -- with a dozen integer operations a run and no cross-lane traffic.  WIDE (maxOps % 4 == 0: a row is 16-byte
 * aligned) reads the row in 16-byte loads, four runs each; other values of maxOps take dword loads.  The walk checks the runs,
 * sums the read and the text length and counts the bytes of both strings in one pass -- the MD's length is a function of the
 * runs alone, so NO text is read here.  It leaves the two lengths (0 and 0: NONE or SKIPPED) in the call's scratch, from where the
 * library's scan makes the offsets, and counts the skipped reads, one atomic per wave that met any.
 *
 * WRITE.  A WAVE owns 64 consecutive reads, hence ONE contiguous span of each arena: [offsets[first], offsets[r + 1]) of its last
 * read that fits the capacity (the reads that fit are a prefix: the offsets ascend).  Two tiers per wave and string:
 *   tile    (span <= kStringsTileBytes) every lane formats its string into the wave's LDS tile at offsets[r] - offsets[first] +
 *           skew, skew = the span's first address & 3, so that LDS word w is the dword at (span's first address & ~3) + 4 w; the
 *           wave then stores the span in whole dwords, consecutive lanes consecutive dwords -- except the first and the last
 *           word where the span does not fill them: those bytes go out as byte stores, for a dword there would overwrite the
 *           neighbouring wave's bytes (or the caller's, beyond the arena);
 *   direct  (a larger span -- scripts of many runs, a long D -- or $AWFM_GPU_DIAG strings_tier=direct) every lane stores its
 *           string's bytes where they go.
 * One formatter, stringsCigar / stringsMd, for both tiers and for the count (COUNT: no stores, no text), so that a length and the
 * bytes behind it cannot disagree.  Only reads with strings load text, and every load of it is the aligned dword that holds the
 * byte asked for -- a byte of the read's record; the text's allocation begins and ends on a 16-byte boundary.  Vector loads and
 * stores only, no scratch, no spill (tests/test_alignment_strings_resources.py holds the unit to kStringsLdsBytes and
 * kStringsMaxVgprs).
 */
#ifndef AWFM_STRINGS_KERNEL_H
#define AWFM_STRINGS_KERNEL_H

#include "awfm_device.h"

namespace {

constexpr unsigned kStringsThreads = 256;     /* per workgroup: four waves, 64 reads each */
constexpr unsigned kStringsTileBytes = 8192;  /* the largest span a wave formats in LDS: 128 bytes a read */
constexpr unsigned kStringsTileWords = 2049;  /* (kStringsTileBytes + a skew of up to 3) / 4, rounded up */
constexpr unsigned kStringsLdsBytes = 32784;  /* four tiles: 4 * kStringsTileWords * 4 -- four workgroups on a CU's 160 KB */
constexpr unsigned kStringsMaxVgprs = 128;    /* four waves a SIMD: what four workgroups a CU, the LDS's limit, come to */
constexpr unsigned long long kStringsMaxRead = AWFM_ALIGN_MAX_LENGTH, kStringsMaxText = 2ull * AWFM_ALIGN_MAX_LENGTH;

static_assert(kStringsTileWords * 4u >= kStringsTileBytes + 3u, "a span of the tile's size at any skew");
static_assert(kStringsLdsBytes == (kStringsThreads / 64u) * kStringsTileWords * 4u, "a tile per wave");

struct DevStringParams {
  struct AwFmStringInputs in;
  struct AwFmStringOutputs out;
  const unsigned char *text;
  const unsigned long long *ends;
  unsigned long long length, numReads;
  unsigned *cigarLengths, *mdLengths; /* [numReads] each, in the call's scratch */
  unsigned numRecords, slots, maxOps, classic, amino, direct;
};

/* run i of a row: four runs a 16-byte load, or a dword load a run */
template <bool WIDE>
struct StringsRow {
  const unsigned *row;
  uint4 four;
  __device__ __forceinline__ unsigned at(const unsigned i) {
    if (!WIDE) return row[i];
    if ((i & 3u) == 0u) four = ((const uint4 *)row)[i >> 2];
    const unsigned which = i & 3u;
    return which == 0u ? four.x : which == 1u ? four.y : which == 2u ? four.z : four.w;
  }
};

__device__ __forceinline__ unsigned stringsDigits(const unsigned v) {
  return v < 10u ? 1u : v < 100u ? 2u : v < 1000u ? 3u : v < 10000u ? 4u : v < 100000u ? 5u : v < 1000000u ? 6u : v < 10000000u ? 7u : v < 100000000u ? 8u : v < 1000000000u ? 9u : 10u;
}

/* `value` in decimal without leading zeros at dst + at; returns where it ends */
template <bool COUNT>
__device__ __forceinline__ unsigned stringsDecimal(unsigned char *dst, const unsigned at, unsigned value) {
  const unsigned digits = stringsDigits(value);
  if (!COUNT) {
    for (unsigned d = digits; d > 0u; d--, value /= 10u) dst[at + d - 1u] = (unsigned char)('0' + value % 10u);
  }
  return at + digits;
}

template <bool COUNT>
__device__ __forceinline__ unsigned stringsByte(unsigned char *dst, const unsigned at, const unsigned c) {
  if (!COUNT) dst[at] = (unsigned char)c;
  return at + 1u;
}

__device__ __forceinline__ unsigned stringsLetter(const unsigned c, const unsigned amino) {
  if (c - 'a' < 26u) return c - 'a' + 'A';
  if (c - 'A' < 26u) return c;
  return amino ? 'X' : 'N';
}

/* text[p] from the aligned dword that holds it; `held` is the address of the dword in `word` (0: none) */
__device__ __forceinline__ unsigned stringsTextByte(const unsigned char *text, const unsigned long long p, unsigned long long &held, unsigned &word) {
  const unsigned char *at = text + p;
  const unsigned skew = (unsigned)((unsigned long long)at & 3ull);
  const unsigned long long base = (unsigned long long)at - skew;
  if (base != held) {
    word = *(const unsigned *)(at - skew);
    held = base;
  }
  return (word >> (8u * skew)) & 0xFFu;
}

__device__ __forceinline__ unsigned stringsOpLetter(const unsigned op) { return op == 1u ? 'I' : op == 2u ? 'D' : op == 4u ? 'S' : op == 7u ? '=' : 'X'; }

/* the CIGAR of a checked row; classic: runs of '=' and 'X' next to each other are one M */
template <bool WIDE, bool COUNT>
__device__ __forceinline__ unsigned stringsCigar(const unsigned *rowAt, const unsigned k, const unsigned classic, unsigned char *dst) {
  StringsRow<WIDE> row{rowAt, {}};
  unsigned at = 0, merged = 0;
  for (unsigned i = 0; i < k; i++) {
    const unsigned run = row.at(i), len = run >> 4, op = run & 15u;
    if (classic && op >= 7u) {
      merged += len;
      continue;
    }
    if (merged) {
      at = stringsByte<COUNT>(dst, stringsDecimal<COUNT>(dst, at, merged), 'M');
      merged = 0;
    }
    at = stringsByte<COUNT>(dst, stringsDecimal<COUNT>(dst, at, len), stringsOpLetter(op));
  }
  if (merged) at = stringsByte<COUNT>(dst, stringsDecimal<COUNT>(dst, at, merged), 'M');
  return at;
}

/* the MD of a checked row whose text begins at text + p; COUNT reads no text */
template <bool WIDE, bool COUNT>
__device__ __forceinline__ unsigned stringsMd(const unsigned *rowAt, const unsigned k, const unsigned char *text, unsigned long long p,
                                              const unsigned amino, unsigned char *dst) {
  StringsRow<WIDE> row{rowAt, {}};
  unsigned long long held = 0;
  unsigned word = 0, at = 0, m = 0;
  for (unsigned i = 0; i < k; i++) {
    const unsigned run = row.at(i), len = run >> 4, op = run & 15u;
    if (op == 7u) {
      m += len;
      p += len;
    } else if (op == 8u) {
      if (COUNT) {
        at += stringsDigits(m) + 1u + 2u * (len - 1u); /* m and a letter, then "0" and a letter for each of the others */
      } else {
        for (unsigned c = 0; c < len; c++, p++) {
          at = stringsByte<COUNT>(dst, stringsDecimal<COUNT>(dst, at, m), stringsLetter(stringsTextByte(text, p, held, word), amino));
          m = 0;
        }
      }
      m = 0;
    } else if (op == 2u) {
      at = stringsByte<COUNT>(dst, stringsDecimal<COUNT>(dst, at, m), '^');
      if (COUNT) {
        at += len;
      } else {
        for (unsigned c = 0; c < len; c++, p++) at = stringsByte<COUNT>(dst, at, stringsLetter(stringsTextByte(text, p, held, word), amino));
      }
      m = 0;
    }
  }
  return stringsDecimal<COUNT>(dst, at, m);
}

/* where the text of read r's script begins (global), for a read the lengths kernel gave strings: all checks have passed */
__device__ __forceinline__ unsigned long long stringsTextAt(const DevStringParams &p, const unsigned long long r) {
  const unsigned s = p.in.sequences[r * p.slots + p.in.slots[r]];
  const unsigned long long S = p.numRecords && s ? p.ends[s - 1u] + 1ull : 0ull;
  return S + p.in.textBegins[r];
}

template <bool WIDE>
__global__ void __launch_bounds__(kStringsThreads) stringLengthsKernel(const DevStringParams p) {
  const unsigned long long r = (unsigned long long)blockIdx.x * kStringsThreads + threadIdx.x;
  unsigned skipped = 0;
  if (r < p.numReads) {
    const unsigned k = p.in.numOps[r];
    unsigned cigar = 0, md = 0;
    if (k != 0u) {
      /* SKIPPED unless every check passes, in the header's order; a row is read only when it is whole */
      bool good = k <= p.maxOps;
      const unsigned j = good ? p.in.slots[r] : 0u;
      good = good && j < p.slots;
      const unsigned s = good ? p.in.sequences[r * p.slots + j] : 0u;
      good = good && s < (p.numRecords ? p.numRecords : 1u);
      unsigned long long L = 0;
      if (good) {
        const unsigned long long E = p.numRecords ? p.ends[s] : p.length, S = p.numRecords && s ? p.ends[s - 1u] + 1ull : 0ull;
        good = !(p.numRecords && s && S == 0ull) && E >= S && E <= p.length;
        L = E - S;
      }
      if (good) {
        const unsigned *rowAt = p.in.ops + r * p.maxOps;
        StringsRow<WIDE> row{rowAt, {}};
        unsigned long long readLength = 0, textLength = 0;
        for (unsigned i = 0; i < k; i++) {
          const unsigned run = row.at(i), len = run >> 4, op = run & 15u;
          good = good && len != 0u && (op == 1u || op == 2u || op == 4u || op == 7u || op == 8u);
          readLength += op != 2u ? len : 0u;
          textLength += op == 2u || op >= 7u ? len : 0u;
        }
        const unsigned long long begin = p.in.textBegins[r];
        good = good && readLength <= kStringsMaxRead && textLength <= kStringsMaxText && begin <= L && textLength <= L - begin;
        if (good) { /* (lengths below 2^18 from here on: 32 bits hold every number the strings carry) */
          cigar = stringsCigar<WIDE, true>(rowAt, k, p.classic, nullptr);
          md = stringsMd<WIDE, true>(rowAt, k, nullptr, 0ull, p.amino, nullptr);
        }
      }
      skipped = good ? 0u : 1u;
    }
    p.cigarLengths[r] = cigar;
    p.mdLengths[r] = md;
  }
  const unsigned long long met = __builtin_amdgcn_ballot_w64(skipped != 0u);
  if ((threadIdx.x & 63u) == 0u && met != 0ull && p.out.numSkipped) atomicAdd((unsigned long long *)p.out.numSkipped, (unsigned long long)__builtin_popcountll(met));
}

__device__ __forceinline__ unsigned long long stringsWaveMax(unsigned long long x) {
#pragma unroll
  for (int offset = 32; offset > 0; offset >>= 1) {
    const unsigned low = (unsigned)__shfl_xor((int)(unsigned)x, offset, 64), high = (unsigned)__shfl_xor((int)(unsigned)(x >> 32), offset, 64);
    const unsigned long long other = ((unsigned long long)high << 32) | low;
    x = other > x ? other : x;
  }
  return x;
}

/* One string of the wave's 64 reads into its arena.  mine: this lane's read has a string and it fits the capacity; from, to: its
 * place in the arena.  MD: the MD, else the CIGAR */
template <bool WIDE, bool MD>
__device__ __forceinline__ void stringsStoreSpan(const DevStringParams &p, unsigned *tile, unsigned char *arena, const bool mine,
                                                 const unsigned long long from, const unsigned long long to, const unsigned long long r,
                                                 const unsigned k, const unsigned lane) {
  /* the span: from the first lane's `from` (every lane's when it has no string: offsets[r]) to the last fitting lane's `to` */
  const unsigned long long spanBegin = ((unsigned long long)(unsigned)__shfl((int)(unsigned)(from >> 32), 0, 64) << 32) | (unsigned)__shfl((int)(unsigned)from, 0, 64);
  const unsigned long long spanEnd = stringsWaveMax(mine ? to : spanBegin);
  const unsigned long long bytes = spanEnd - spanBegin;
  if (bytes == 0ull) return; /* (the same in every lane) */
  const unsigned *rowAt = p.in.ops + r * p.maxOps;
  if (bytes > kStringsTileBytes || p.direct) {
    if (mine) {
      if (MD) stringsMd<WIDE, false>(rowAt, k, p.text, stringsTextAt(p, r), p.amino, arena + from);
      else stringsCigar<WIDE, false>(rowAt, k, p.classic, arena + from);
    }
    return;
  }
  const unsigned skew = (unsigned)((unsigned long long)(arena + spanBegin) & 3ull), end = skew + (unsigned)bytes;
  __builtin_amdgcn_wave_barrier(); /* (the stores of the string before have read the tile) */
  if (mine) {
    unsigned char *dst = (unsigned char *)tile + skew + (unsigned)(from - spanBegin);
    if (MD) stringsMd<WIDE, false>(rowAt, k, p.text, stringsTextAt(p, r), p.amino, dst);
    else stringsCigar<WIDE, false>(rowAt, k, p.classic, dst);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  /* word w of the tile is the dword at base + 4 w; bytes [skew, end) of the tile are the span */
  unsigned char *base = arena + spanBegin - skew;
  const unsigned words = (end + 3u) >> 2;
  for (unsigned w = lane; w < words; w += 64u) {
    const unsigned lo = 4u * w < skew ? skew : 4u * w, hi = 4u * w + 4u > end ? end : 4u * w + 4u;
    if (hi - lo == 4u) {
      ((unsigned *)base)[w] = tile[w];
    } else {
      for (unsigned b = lo; b < hi; b++) base[b] = ((const unsigned char *)tile)[b];
    }
  }
}

template <bool WIDE>
__global__ void __launch_bounds__(kStringsThreads) stringWriteKernel(const DevStringParams p) {
  __shared__ unsigned tiles[kStringsThreads / 64u][kStringsTileWords];
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x / 64u;
  const unsigned long long first = (unsigned long long)blockIdx.x * kStringsThreads + (threadIdx.x & ~63u);
  if (first >= p.numReads) return; /* (the whole wave) */
  const bool inBatch = first + lane < p.numReads;
  const unsigned long long r = inBatch ? first + lane : p.numReads - 1ull; /* a lane beyond the batch looks at the last read and has no string */
  const bool has = inBatch && p.cigarLengths[r] != 0u; /* (a read with strings has a run, hence a CIGAR) */
  const unsigned k = has ? p.in.numOps[r] : 0u;
  bool missed = false;
  if (p.out.cigarChars) {
    const unsigned long long from = p.out.cigarOffsets[r], to = p.out.cigarOffsets[r + 1ull];
    const bool fits = to <= p.out.cigarCapacity;
    missed = missed || (has && !fits);
    stringsStoreSpan<WIDE, false>(p, tiles[wave], p.out.cigarChars, has && fits, from, to, r, k, lane);
  }
  if (p.out.mdChars) {
    const unsigned long long from = p.out.mdOffsets[r], to = p.out.mdOffsets[r + 1ull];
    const bool fits = to <= p.out.mdCapacity;
    missed = missed || (has && !fits);
    stringsStoreSpan<WIDE, true>(p, tiles[wave], p.out.mdChars, has && fits, from, to, r, k, lane);
  }
  const unsigned long long met = __builtin_amdgcn_ballot_w64(missed);
  if (lane == 0u && met != 0ull && p.out.numOverflow) atomicAdd((unsigned long long *)p.out.numOverflow, (unsigned long long)__builtin_popcountll(met));
}

}  // namespace

#endif
