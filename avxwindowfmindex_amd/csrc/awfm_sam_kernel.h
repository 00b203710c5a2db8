/*
 * awfm_sam_kernel.h -- samLengthsKernel and samWriteKernel, the kernels of "SAM records" (include/awfm_gpu.h).  The definition is
 * the header's; the host twin and checker is awfm_sam.c.
 *
 * ONE description of a line serves both kernels: samReadOf gathers what a read's line depends on (its own values and the few of
 * its mate's), and samFieldOf turns that into field f of kSamFields: absent, a byte, a decimal number or a run of bytes to
 * copy, with an optional five-character tag in front.  A field's bytes are a tab (all but the first), the tag, the body; the
 * line ends in '\n'.  So a length and the bytes behind it cannot disagree.
 *
 * LENGTHS.  A THREAD takes a read and adds up its fields' bytes: field lengths and digit counts (comparisons, no division),
 * no byte of a read, a name or a string is loaded.  It leaves the length in the call's scratch, from where the library's scan
 * makes lineOffsets, and counts the unaligned reads, one atomic per wave that met any.
 *
 * WRITE.  A WAVE takes a read: a line is 300 to 500 bytes on the measured batch, several times a wave's width, and its pieces
 * lie in six different arrays; 64 reads a wave as in awfm_strings_kernel.h would have every lane walk its own 400 bytes.  Lane
 * f owns field f: it computes the field's bytes, a prefix sum over the lanes gives every field its place, and the owner writes
 * the tab, the tag and the digits (made in registers) or the byte.  The runs -- QNAME, RNAME, CIGAR, RNEXT, SEQ, QUAL, MD -- are
 * then copied by all lanes, lane-consecutive bytes.  Two tiers:
 *   tile    (the line and its skew fit kSamTileBytes) the line is built in the wave's LDS tile at skew = its first address & 3, so
 *           that LDS word w is the dword at (first address & ~3) + 4 w; the wave then stores whole dwords, consecutive lanes
 *           consecutive dwords -- except the first and the last word where the line does not fill them: those bytes go out as
 *           byte stores, for a dword there would overwrite the neighbouring line's bytes (or the caller's, beyond the arena);
 *   direct  (a longer line, or $AWFM_GPU_DIAG sam_tier=direct) the same stores go straight to the arena.
 * A line is written only when lineOffsets[r + 1] <= lineCapacity; else lane 0 counts it.  Vector loads and stores only, no
 * scratch, no spill (tests/test_sam_records_resources.py holds the unit to kSamLdsBytes and kSamMaxVgprs).
 */
#ifndef AWFM_SAM_KERNEL_H
#define AWFM_SAM_KERNEL_H

#include "awfm_device.h"

namespace {

constexpr unsigned kSamThreads = 256;    /* per workgroup: 256 reads in the lengths kernel, four waves = four reads in the write kernel */
constexpr unsigned kSamTileBytes = 2048; /* the longest line (with its skew) a wave builds in LDS: reads of up to ~950 characters with qualities */
constexpr unsigned kSamTileWords = 512;  /* kSamTileBytes / 4 */
constexpr unsigned kSamLdsBytes = 8192;  /* four tiles */
constexpr unsigned kSamMaxVgprs = 64;    /* eight waves a SIMD */
constexpr unsigned kSamFields = 15;      /* QNAME FLAG RNAME POS MAPQ CIGAR RNEXT PNEXT TLEN SEQ QUAL NM AS XS MD */

static_assert(kSamTileWords * 4u == kSamTileBytes, "whole words");
static_assert(kSamLdsBytes == (kSamThreads / 64u) * kSamTileWords * 4u, "a tile per wave");
static_assert(kSamFields <= 64u, "a lane per field");

enum : unsigned { kSamAbsent = 0, kSamByte = 1, kSamDecimal = 2, kSamCopy = 3 };

struct DevSamParams {
  struct AwFmSamInputs in;
  struct AwFmSamOutputs out;
  unsigned long long numReads;
  unsigned *lengths; /* [numReads], in the call's scratch */
  unsigned slots, paired, direct;
};

/* what the line of read r depends on */
struct SamRead {
  unsigned long long r, m, n; /* the read, its mate (r ^ 1), its length */
  unsigned s, sm, place;      /* the read's record, the mate's, the one RNAME names */
  bool aligned, mateAligned;
};

struct SamField {
  const unsigned char *src; /* kSamCopy */
  unsigned long long value; /* kSamDecimal: the magnitude */
  unsigned length;          /* the body's bytes: the run's, the digits and the sign, 1 */
  unsigned kind;
  unsigned c;   /* kSamByte: the byte; kSamDecimal: 1 when negative */
  unsigned tag; /* 0, or the tag's two letters and its type: 'N' | 'M' << 8 | 'i' << 16 */
};

__device__ __forceinline__ unsigned samDigits(const unsigned long long v) {
  unsigned d = 1u;
  unsigned long long bound = 10ull;
#pragma unroll
  for (int i = 0; i < 19; i++, bound *= 10ull) d += v >= bound ? 1u : 0u; /* (unrolled: nineteen constants) */
  return d;
}

/* ALIGNED or not, by the header's list; s: the record */
__device__ __forceinline__ bool samIsAligned(const DevSamParams &p, const unsigned long long r, unsigned &s) {
  const unsigned score = p.in.scores[r], j = p.in.slots[r];
  s = 0u;
  if (score == 0u || score >= AWFM_VERIFY_TOO_LONG || j >= p.slots) return false;
  s = p.in.sequences[r * p.slots + j];
  return s < p.in.numRecordNames && p.in.readOffsets[r + 1ull] >= p.in.readOffsets[r];
}

__device__ __forceinline__ SamRead samReadOf(const DevSamParams &p, const unsigned long long r) {
  SamRead rd;
  rd.r = r;
  rd.m = r ^ 1ull;
  rd.aligned = samIsAligned(p, r, rd.s);
  rd.sm = 0u;
  rd.mateAligned = p.paired && samIsAligned(p, rd.m, rd.sm);
  rd.place = rd.aligned ? rd.s : rd.sm;
  const unsigned long long begin = p.in.readOffsets[r], end = p.in.readOffsets[r + 1ull];
  rd.n = end >= begin ? end - begin : 0ull;
  return rd;
}

__device__ __forceinline__ SamField samByteField(const unsigned c) { return SamField{nullptr, 0ull, 1u, kSamByte, c, 0u}; }
__device__ __forceinline__ SamField samDecimalField(const unsigned long long v, const unsigned tag) {
  return SamField{nullptr, v, samDigits(v), kSamDecimal, 0u, tag};
}
/* the bytes [offsets[i], offsets[i + 1]) of an arena */
__device__ __forceinline__ SamField samRunField(const unsigned char *chars, const uint64_t *offsets, const unsigned long long i,
                                                const unsigned tag) {
  const unsigned long long from = offsets[i];
  return SamField{chars + from, 0ull, (unsigned)(offsets[i + 1ull] - from), kSamCopy, 0u, tag};
}
__device__ __forceinline__ SamField samRunOrStar(const SamField run) { return run.length ? run : samByteField('*'); }
__device__ __forceinline__ constexpr unsigned samTag(const char a, const char b, const char type) {
  return (unsigned)a | (unsigned)b << 8 | (unsigned)type << 16;
}

/* field f of the line */
__device__ __forceinline__ SamField samFieldOf(const DevSamParams &p, const SamRead &rd, const unsigned f) {
  const SamField absent{nullptr, 0ull, 0u, kSamAbsent, 0u, 0u};
  const unsigned long long r = rd.r, m = rd.m;
  const bool placed = rd.aligned || rd.mateAligned;
  switch (f) {
    case 0: /* QNAME */
      if (p.in.nameOffsets) return samRunField(p.in.nameChars, p.in.nameOffsets, r, 0u);
      return samDecimalField(p.paired ? r >> 1 : r, 0u);
    case 1: { /* FLAG */
      unsigned flag = p.in.baseFlags ? p.in.baseFlags[r] : 0u;
      if (!rd.aligned) flag |= 0x4u;
      if (p.paired) {
        flag |= 0x1u | ((r & 1ull) ? 0x80u : 0x40u);
        if (p.in.properPairs && rd.aligned && rd.mateAligned && p.in.properPairs[r >> 1]) flag |= 0x2u;
        if (!rd.mateAligned) flag |= 0x8u;
        if (p.in.baseFlags && (p.in.baseFlags[m] & 0x10u)) flag |= 0x20u;
      }
      return samDecimalField(flag, 0u);
    }
    case 2: /* RNAME */
      return placed ? samRunField(p.in.recordNameChars, p.in.recordNameOffsets, rd.place, 0u) : samByteField('*');
    case 3: /* POS */
      return samDecimalField(placed ? p.in.textBegins[rd.aligned ? r : m] + 1ull : 0ull, 0u);
    case 4: /* MAPQ */
      return samDecimalField(rd.aligned ? (p.in.mappingQualities ? p.in.mappingQualities[r] : 255u) : 0u, 0u);
    case 5: /* CIGAR */
      return rd.aligned ? samRunOrStar(samRunField(p.in.cigarChars, p.in.cigarOffsets, r, 0u)) : samByteField('*');
    case 6: /* RNEXT */
      if (!rd.mateAligned) return samByteField('*');
      if (rd.place == rd.sm) return samByteField('=');
      return samRunField(p.in.recordNameChars, p.in.recordNameOffsets, rd.sm, 0u);
    case 7: /* PNEXT */
      return samDecimalField(rd.mateAligned ? p.in.textBegins[m] + 1ull : 0ull, 0u);
    case 8: { /* TLEN */
      unsigned long long span = 0ull;
      if (rd.aligned && rd.mateAligned && rd.s == rd.sm) {
        const unsigned long long mine = p.in.textBegins[r], mates = p.in.textBegins[m], myEnd = p.in.textEnds[r], matesEnd = p.in.textEnds[m];
        const unsigned long long b = mine < mates ? mine : mates, e = myEnd > matesEnd ? myEnd : matesEnd;
        const bool first = mine < mates || (mine == mates && (r & 1ull) == 0ull);
        span = first ? e - b : 0ull - (e - b); /* 64-bit two's complement */
      }
      const bool negative = (span >> 63) != 0ull;
      SamField field = samDecimalField(negative ? 0ull - span : span, 0u);
      field.c = negative ? 1u : 0u;
      field.length += field.c;
      return field;
    }
    case 9: /* SEQ */
      return rd.n ? SamField{p.in.readChars + p.in.readOffsets[r], 0ull, (unsigned)rd.n, kSamCopy, 0u, 0u} : samByteField('*');
    case 10: /* QUAL */
      return p.in.qualities && rd.n ? SamField{p.in.qualities + p.in.readOffsets[r], 0ull, (unsigned)rd.n, kSamCopy, 0u, 0u} : samByteField('*');
    case 11: /* NM */
      return rd.aligned ? samDecimalField(p.in.editDistances[r], samTag('N', 'M', 'i')) : absent;
    case 12: /* AS */
      return rd.aligned ? samDecimalField(p.in.scores[r], samTag('A', 'S', 'i')) : absent;
    case 13: /* XS */
      return rd.aligned && p.in.secondScores ? samDecimalField(p.in.secondScores[r], samTag('X', 'S', 'i')) : absent;
    case 14: { /* MD */
      if (!rd.aligned || !p.in.mdOffsets) return absent;
      const SamField run = samRunField(p.in.mdChars, p.in.mdOffsets, r, samTag('M', 'D', 'Z'));
      return run.length ? run : absent;
    }
    default:
      return absent;
  }
}

/* the bytes of field f before its body: the tab and the tag */
__device__ __forceinline__ unsigned samLeadBytes(const SamField &field, const unsigned f) {
  return field.kind == kSamAbsent ? 0u : (f != 0u ? 1u : 0u) + (field.tag ? 5u : 0u);
}
__device__ __forceinline__ unsigned samFieldBytes(const SamField &field, const unsigned f) {
  return field.kind == kSamAbsent ? 0u : samLeadBytes(field, f) + field.length;
}

__global__ void __launch_bounds__(kSamThreads) samLengthsKernel(const DevSamParams p) {
  const unsigned long long r = (unsigned long long)blockIdx.x * kSamThreads + threadIdx.x;
  bool unaligned = false;
  if (r < p.numReads) {
    const SamRead rd = samReadOf(p, r);
    unsigned total = 1u; /* '\n' */
#pragma unroll
    for (unsigned f = 0; f < kSamFields; f++) total += samFieldBytes(samFieldOf(p, rd, f), f);
    p.lengths[r] = total;
    unaligned = !rd.aligned;
  }
  const unsigned long long met = __builtin_amdgcn_ballot_w64(unaligned);
  if ((threadIdx.x & 63u) == 0u && met != 0ull && p.out.numUnaligned)
    atomicAdd((unsigned long long *)p.out.numUnaligned, (unsigned long long)__builtin_popcountll(met));
}

__device__ __forceinline__ unsigned long long samBroadcast64(const unsigned long long x, const int lane) {
  return ((unsigned long long)(unsigned)__shfl((int)(unsigned)(x >> 32), lane, 64) << 32) | (unsigned)__shfl((int)(unsigned)x, lane, 64);
}

/* The line of the wave's read at dst, `total` bytes: every lane its field's tab, tag and digits or byte; the runs by all lanes */
__device__ __forceinline__ void samFormat(const DevSamParams &p, const SamRead &rd, unsigned char *dst, const unsigned lane, const unsigned total,
                                          const SamField &field, const unsigned start) {
  const unsigned body = start + samLeadBytes(field, lane);
  if (field.kind != kSamAbsent) {
    unsigned at = start;
    if (lane != 0u) dst[at++] = '\t';
    if (field.tag) {
      dst[at] = (unsigned char)(field.tag & 0xFFu);
      dst[at + 1u] = (unsigned char)((field.tag >> 8) & 0xFFu);
      dst[at + 2u] = ':';
      dst[at + 3u] = (unsigned char)(field.tag >> 16);
      dst[at + 4u] = ':';
    }
    if (field.kind == kSamByte) dst[body] = (unsigned char)field.c;
    if (field.kind == kSamDecimal) {
      if (field.c) dst[body] = '-';
      unsigned long long v = field.value;
      for (unsigned d = field.length; d > field.c; d--, v /= 10ull) dst[body + d - 1u] = (unsigned char)('0' + (unsigned)(v % 10ull));
    }
  }
  if (lane == kSamFields) dst[total - 1u] = '\n';
#pragma unroll
  for (unsigned f = 0; f < kSamFields; f++) {
    if (f == 1u || f == 3u || f == 4u || f == 7u || f == 8u || (f >= 11u && f <= 13u)) continue; /* never a run */
    if ((unsigned)__shfl((int)field.kind, (int)f, 64) != kSamCopy) continue;                     /* (the same in every lane) */
    const unsigned char *src = (const unsigned char *)samBroadcast64((unsigned long long)field.src, (int)f);
    const unsigned length = (unsigned)__shfl((int)field.length, (int)f, 64), to = (unsigned)__shfl((int)body, (int)f, 64);
    for (unsigned i = lane; i < length; i += 64u) dst[to + i] = src[i];
  }
}

__global__ void __launch_bounds__(kSamThreads) samWriteKernel(const DevSamParams p) {
  __shared__ unsigned tiles[kSamThreads / 64u][kSamTileWords];
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x / 64u;
  const unsigned long long r = (unsigned long long)blockIdx.x * (kSamThreads / 64u) + wave;
  if (r >= p.numReads) return; /* (the whole wave) */
  const unsigned long long from = p.out.lineOffsets[r], to = p.out.lineOffsets[r + 1ull];
  if (to > p.out.lineCapacity) {
    if (lane == 0u && p.out.numOverflow) atomicAdd((unsigned long long *)p.out.numOverflow, 1ull);
    return;
  }
  const SamRead rd = samReadOf(p, r);
  const SamField field = samFieldOf(p, rd, lane);
  const unsigned bytes = samFieldBytes(field, lane);
  unsigned sum = bytes; /* the inclusive prefix sum over the lanes */
#pragma unroll
  for (int offset = 1; offset < 16; offset <<= 1) { /* (lanes from kSamFields on hold 0: sixteen lanes carry all of it) */
    const unsigned below = (unsigned)__shfl_up((int)sum, offset, 64);
    if (lane >= (unsigned)offset) sum += below;
  }
  const unsigned total = (unsigned)__shfl((int)sum, 15, 64) + 1u;
  if ((unsigned long long)total != to - from) return; /* the offsets are this call's own: never, and then no byte is stored */
  unsigned char *line = p.out.lineChars + from;
  const unsigned skew = (unsigned)((unsigned long long)line & 3ull), end = skew + total;
  if (end > kSamTileBytes || p.direct) {
    samFormat(p, rd, line, lane, total, field, sum - bytes);
    return;
  }
  unsigned *tile = tiles[wave];
  samFormat(p, rd, (unsigned char *)tile + skew, lane, total, field, sum - bytes);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  /* word w of the tile is the dword at base + 4 w; bytes [skew, end) of the tile are the line */
  unsigned char *base = line - skew;
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

}  // namespace

#endif
