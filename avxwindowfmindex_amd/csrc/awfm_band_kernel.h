/*
 * awfm_band_kernel.h -- what the kernels of the read path share (awfm_verify_kernel.h, awfm_align_kernel.h,
 * awfm_align_affine_kernel.h, awfm_score_affine_kernel.h, awfm_matrix_kernel.h, awfm_end_bonus_kernel.h; awfm_window_affine_kernel.h takes the letters): a group's staging of
 * read and text bytes into LDS, the letter comparison, the classification of a chain slot up to TOO WIDE, the band of a whole
 * read and the staging of one of its chunks, the row and the end cell of the banded affine recurrence, the two sources of the
 * diagonal's score (two costs, or a substitution matrix in LDS) -- and what their
 * launchers share: the argument checks with their messages, the choice of the lanes per group and the dispatch over it.  The
 * host's definitions of the same things are awfm_band.h.
 *
 * EVERY READ OF THE TEXT AND OF THE READ BUFFER by these kernels is an aligned dword that holds at least one byte of the interval
 * the slot owns: stageBytes is the one place that forms such an address.  The text's allocation ends on a 16-byte boundary
 * beyond its last byte and begins on one, so such a dword lies inside it; a dword of the read buffer that holds a byte of the
 * buffer lies in that byte's page.
 *
 * The functions take the launch's parameters as `const P &`: a kernel that keeps them in the argument segment passes that, one
 * that has copied them and pinned fields into vector registers passes its copy.  Vector loads and stores only.
 */
#ifndef AWFM_BAND_KERNEL_H
#define AWFM_BAND_KERNEL_H

#include "awfm_device.h"

namespace {

constexpr unsigned kVerifyChunk = 64;       /* rows per staging */
constexpr unsigned kVerifyReadWords = 18;   /* 64 characters at any skew: 17 aligned dwords */
constexpr unsigned kVerifyTextWords = 34;   /* 64 + 63 characters at any skew: 33 aligned dwords */
constexpr unsigned kVerifyGroupWords = 52;  /* a group's staging words: read, then text */
static_assert(kVerifyGroupWords == kVerifyReadWords + kVerifyTextWords, "read words, then text words");
constexpr int kVerifyInf = 0x3FFFFFFF;      /* a cell of the unit-cost rows that is outside the matrix or the band */
constexpr int kBandNeg = -0x40000000;       /* minus infinity of the affine rows: a lane resets it every row, so it only has to survive o + 64 e */
constexpr unsigned kSlotHasBand = 0u;       /* what classifySlot returns for a slot without a status */

/* bytes [from, to) of `base`, to > from, to - from <= the words given, into the group's LDS words with aligned dword loads
 * of dwords that hold one of those bytes; returns where byte `from` lies in them */
template <int G>
__device__ __forceinline__ unsigned stageBytes(const unsigned char *base, unsigned long long from, unsigned long long to, unsigned *words,
                                               unsigned k) {
  const unsigned long long a = (unsigned long long)(base + from), first = a & ~3ull, last = ((unsigned long long)(base + to) + 3ull) & ~3ull;
  const unsigned count = (unsigned)((last - first) >> 2);
  const unsigned *src = (const unsigned *)first;
  for (unsigned w = k; w < count; w += (unsigned)G) words[w] = src[w];
  return (unsigned)(a - first);
}

__device__ __forceinline__ unsigned verifyLetter(const unsigned char *sAmino, unsigned amino, unsigned c) {
  return amino ? (c == '$' ? 21u : (unsigned)sAmino[c & 31u]) : nucLetterIndex(c);
}

/* a classified slot that has a band: its record [S, S + L), its read interval and where that begins in the record */
struct SlotBand {
  unsigned long long S, rb, re;
  long long L, tb, bD, eD;
};

/* Slot `at` (sequence s) of a read of readLength characters whose offsets are good or not: AWFM_VERIFY_NONE, MALFORMED or
 * TOO_WIDE in the order the header lists the checks, or kSlotHasBand with b.  The caller goes on with what is its own: TOO LONG,
 * OVERHANG, the band.  awfmGpuIndexSetRecordTable (awfmGpuInstallRecordTable) takes no end of 2^62 or more, so E - S < 2^62 and
 * the device needs no check for a record end of 2^64 - 1, which the host's awfmRecordBounds has */
template <typename P>
__device__ __forceinline__ unsigned classifySlot(const P &p, const unsigned long long at, const unsigned s, const unsigned long long readLength,
                                                 const bool readOk, SlotBand &b) {
  if (s == AWFM_CANDIDATES_NONE || p.in.chainAnchors[at] == 0u) return AWFM_VERIFY_NONE;
  if (!readOk) return AWFM_VERIFY_MALFORMED;
  b.rb = p.in.chainReadBegins[at];
  b.re = p.in.chainReadEnds[at];
  if (b.rb > b.re || b.re > readLength) return AWFM_VERIFY_MALFORMED;
  if (s >= (p.numRecords ? p.numRecords : 1u)) return AWFM_VERIFY_MALFORMED;
  const unsigned long long E = p.numRecords ? p.ends[s] : p.length;
  b.S = p.numRecords && s ? p.ends[s - 1u] + 1ull : 0ull;
  if (E < b.S || E > p.length) return AWFM_VERIFY_MALFORMED;
  b.bD = p.in.chainBeginDiagonals[at];
  b.eD = p.in.chainEndDiagonals[at];
  /* E - S < 2^62 and rb, re < 2^32: a diagonal outside [-2^33, 2^62] makes tb < 0, tb > te or te > E - S whatever the other is,
   * and inside it the sums are exact in 64 bits */
  if (b.bD < -(1ll << 33) || b.eD < -(1ll << 33) || b.bD > (1ll << 62) || b.eD > (1ll << 62)) return AWFM_VERIFY_MALFORMED;
  const long long te = (long long)b.re + b.eD;
  b.tb = (long long)b.rb + b.bD;
  b.L = (long long)(E - b.S);
  if (b.tb < 0 || b.tb > te || te > b.L) return AWFM_VERIFY_MALFORMED;
  const long long delta = b.eD - b.bD;
  if (delta > (long long)p.drift || delta < -(long long)p.drift) return AWFM_VERIFY_TOO_WIDE;
  return kSlotHasBand;
}

/* The band of a whole read of n rows in sequence-local coordinates: the diagonals [lo, hi], and columns counted from lo --
 * lane k's cell of row i is u = i + k, t = lo + u; it exists for uMin <= u <= uMax and k < width.  width, uMin, uMax and uOne
 * mean what they say once the caller has ruled out a band that lies wholly outside the record's rows (then -n - 63 <= lo <= L);
 * what lies beyond 2^30 is beyond every row */
struct ReadBand {
  long long lo, hi;
  int width, uMin, uMax;
  int uOne; /* t >= 1 from here on: the cell has a diagonal predecessor */
};

__device__ __forceinline__ ReadBand readBand(const SlotBand &b, const unsigned pad) {
  ReadBand band;
  band.lo = (b.bD < b.eD ? b.bD : b.eD) - (long long)pad;
  band.hi = (b.bD > b.eD ? b.bD : b.eD) + (long long)pad;
  band.width = (int)(band.hi - band.lo) + 1;
  band.uMin = band.lo < 0 ? (int)-band.lo : 0;
  band.uMax = b.L - band.lo < (1ll << 30) ? (int)(b.L - band.lo) : 1 << 30;
  band.uOne = band.lo < 1 ? (int)(1 - band.lo) : 0;
  return band;
}

/* a staged chunk: where its first read byte and its first text byte lie in the group's words, and which column that text byte is */
struct StagedChunk {
  unsigned rOff, tOff;
  int uFrom;
};

/* The read characters of rows i0 + 1 .. i0 + rows and the text characters T[t - 1] they can touch, u - 1 = i0 .. i0 + rows +
 * width - 2 cut to the record, into the group's words */
template <int G>
__device__ __forceinline__ StagedChunk stageChunk(const unsigned char *R, const unsigned char *T, const ReadBand &band, const int i0, const int rows,
                                                  unsigned *sRead, unsigned *sText, const unsigned k) {
  StagedChunk c;
  c.uFrom = i0 > band.uMin ? i0 : band.uMin;
  const int uTo = i0 + rows + band.width - 1 < band.uMax ? i0 + rows + band.width - 1 : band.uMax;
  __builtin_amdgcn_wave_barrier(); /* (the rows of the chunk before have read their bytes) */
  c.rOff = stageBytes<G>(R, (unsigned long long)i0, (unsigned long long)(i0 + rows), sRead, k);
  c.tOff = uTo > c.uFrom ? stageBytes<G>(T, (unsigned long long)(band.lo + c.uFrom), (unsigned long long)(band.lo + uTo), sText, k) : 0u;
  __builtin_amdgcn_wave_barrier();
  return c;
}

/* the letters of row q of the chunk and of column u; the text's is 0xFF for a cell without a diagonal predecessor */
struct StagedLetters {
  unsigned read, text;
};

__device__ __forceinline__ StagedLetters stagedLetters(const StagedChunk &c, const ReadBand &band, const unsigned *sRead, const unsigned *sText,
                                                       const unsigned char *sAmino, const unsigned amino, const int q, const int u,
                                                       const bool inMatrix) {
  StagedLetters l;
  l.read = verifyLetter(sAmino, amino, ((const unsigned char *)sRead)[c.rOff + (unsigned)q]);
  l.text = 0xFFu;
  if (inMatrix && u >= band.uOne) l.text = verifyLetter(sAmino, amino, ((const unsigned char *)sText)[c.tOff + (unsigned)(u - 1 - c.uFrom)]);
  return l;
}

/* whether they differ: true unless both characters map to the same proper letter, and for a cell without a diagonal predecessor */
__device__ __forceinline__ bool lettersSub(const StagedLetters &l, const unsigned amino) {
  return !(l.read == l.text && l.read < (amino ? 20u : 4u));
}

__device__ __forceinline__ bool stagedSub(const StagedChunk &c, const ReadBand &band, const unsigned *sRead, const unsigned *sText,
                                          const unsigned char *sAmino, const unsigned amino, const int q, const int u, const bool inMatrix) {
  return lettersSub(stagedLetters(c, band, sRead, sText, sAmino, amino, q, u, inMatrix), amino);
}

/* The diagonal's score s(R[i-1], T[t-1]) of a cell, from its two letters and verification's sub: what affineRow adds to the
 * previous row's H.  IdentityScore is "affine alignment"'s, + match or - mismatch out of the launch's parameters.  A scorer also
 * says what a reached read end earns, endBonus(): the constant 0 for these two, so that row 0 starts from 0 and row n's
 * value behind the row loop folds away; "end bonus"' B for EndBonusScore (awfm_end_bonus_kernel.h) */
struct IdentityScore {
  static constexpr __device__ __forceinline__ int endBonus() { return 0; }
  template <typename P>
  __device__ __forceinline__ int operator()(const P &p, const StagedLetters &, const bool sub) const {
    return sub ? -p.mismatch : p.match;
  }
};

/* MatrixScore is "substitution matrices"' (include/awfm_gpu.h): a signed byte out of the workgroup's copy of the launch's matrix in
 * LDS, rows kMatrixStride bytes apart so that a row lies inside 32 bytes -- eight banks.  The class of a letter is the letter
 * capped at `other` (20 or 4): the sentinel, every ambiguity code and the 0xFF of a cell without a diagonal predecessor (whose
 * score meets kBandNeg and counts for nothing) fold into the last class.  The row index is uniform over a group in a row */
constexpr unsigned kMatrixStride = 32;
constexpr unsigned kMatrixLdsBytes = AWFM_MATRIX_CLASSES * kMatrixStride;

struct MatrixScore {
  const signed char *sMatrix;
  unsigned other;
  static constexpr __device__ __forceinline__ int endBonus() { return 0; }
  template <typename P>
  __device__ __forceinline__ int operator()(const P &, const StagedLetters &l, const bool) const {
    const unsigned r = l.read < other ? l.read : other, t = l.text < other ? l.text : other;
    return (int)sMatrix[r * kMatrixStride + t];
  }
};

/* the workgroup's copy of a launch's matrix: `matrix` is the struct's array in the kernel's argument segment; the caller's
 * __syncthreads() follows */
__device__ __forceinline__ void stageMatrix(const __attribute__((address_space(4))) signed char *matrix, signed char *sMatrix) {
  for (unsigned at = threadIdx.x; at < AWFM_MATRIX_CLASSES * AWFM_MATRIX_CLASSES; at += blockDim.x)
    sMatrix[(at / AWFM_MATRIX_CLASSES) * kMatrixStride + at % AWFM_MATRIX_CLASSES] = matrix[at];
}

/* lane k's cell of a row of "affine alignment" */
struct AffineCell {
  int M, F, fOpens, fExtends, e, h;
};

/* A lane carries H and F of the previous row; M comes from the lane itself, F from lane k + 1.  The horizontal value is one
 * exclusive max-prefix-scan per row over the group: E[k] = max over k' < k of (H~[k'] + k' e) - o - k e with H~ = max(0, M, F)
 * -- a gap that extends from a cell whose H came from E pays o twice and is dominated, so the scan's E is the
 * recurrence's.  Lanes and rows without a cell carry kBandNeg and need no other case: max(0, ...) is taken for existing cells
 * only.  p.open is what the first character of a gap costs, o + e; kExtend is k * p.extend; s is the diagonal's score, of
 * IdentityScore or MatrixScore, -128 <= s <= 255.  Neither the scan nor its dominance argument involves s.  kBandNeg survives a
 * row whatever s is: a lane resets it every row, and between two resets it takes one s, o + e and twice 63 e, at most 255 +
 * 510 + 2 * 63 * 255 < 2^16 either way, against 2^30 */
template <int G, typename P>
__device__ __forceinline__ AffineCell affineRow(const P &p, const int prevH, const int prevF, const int s, const bool inMatrix, const int kExtend,
                                                const unsigned k) {
  AffineCell c;
  int upH = __shfl_down(prevH, 1, G), upF = __shfl_down(prevF, 1, G);
  upH = k == (unsigned)(G - 1) ? kBandNeg : upH;
  upF = k == (unsigned)(G - 1) ? kBandNeg : upF;
  c.M = prevH + s; /* (prevH is kBandNeg when t = 0) */
  c.fOpens = upH - p.open;
  c.fExtends = upF - p.extend;
  c.F = c.fOpens > c.fExtends ? c.fOpens : c.fExtends;
  int tilde = c.M > c.F ? c.M : c.F;
  tilde = tilde > 0 ? tilde : 0;
  tilde = inMatrix ? tilde : kBandNeg;
  /* E[k] + o + k e = max over k' < k of H~[k'] + k' e: shifted by a lane, then the inclusive scan */
  int v = __shfl_up(tilde + kExtend, 1, G);
  v = k == 0u ? kBandNeg : v;
#pragma unroll
  for (int step = 1; step < G; step <<= 1) {
    const int other = __shfl_up(v, step, G);
    v = (int)k >= step && other > v ? other : v;
  }
  c.e = v - (p.open - p.extend) - kExtend;
  c.h = inMatrix ? (tilde > c.e ? tilde : c.e) : kBandNeg;
  return c;
}

/* the end cell of the group: the largest H, then the smallest i, then the smallest k, of the lanes' own bests (each the smallest
 * i of the lane's largest H).  H < 2^24, i <= 2^16.  score 0: there is none */
struct AffineEnd {
  unsigned score, i, k;
};

template <int G>
__device__ __forceinline__ AffineEnd affineEndCell(const int bestH, const int bestI, const unsigned k) {
  unsigned long long key = ((unsigned long long)(unsigned)bestH << 32) | ((unsigned long long)(0x1FFFFu - (unsigned)bestI) << 6) | (63u - k);
#pragma unroll
  for (int step = 1; step < G; step <<= 1) {
    const unsigned otherLow = (unsigned)__shfl_xor((int)(unsigned)key, step, G), otherHigh = (unsigned)__shfl_xor((int)(unsigned)(key >> 32), step, G);
    const unsigned long long other = ((unsigned long long)otherHigh << 32) | otherLow;
    key = other > key ? other : key;
  }
  return AffineEnd{(unsigned)(key >> 32), 0x1FFFFu - ((unsigned)(key >> 6) & 0x1FFFFu), 63u - ((unsigned)key & 63u)};
}

/* ---- the launchers (host side) ---- */

/* sets the error `name: what` */
inline void setCallError(const char *name, const char *what) { setError((std::string(name) + ": " + what).c_str()); }

/* What every awfmGpu* call on chain slots refuses after "null image" and numReads == 0, in this order: a null among the inputs
 * (others: the call's own pointers, false when one of them is null), more than 2^32 - 1 reads or a slot count outside 1 .. 16,
 * a band of more than 64 diagonals.  band: maxDrift + 2 bandPad + 1 */
inline enum AwFmReturnCode chainArgumentsRefused(const char *name, const struct AwFmVerifyInputs *dIn, const bool others, const uint64_t numReads,
                                                 const uint32_t maxCandidates, const uint64_t band) {
  if (!dIn || !others || !dIn->readOffsets || !dIn->sequences || !dIn->chainAnchors || !dIn->chainReadBegins || !dIn->chainReadEnds ||
      !dIn->chainBeginDiagonals || !dIn->chainEndDiagonals || (!dIn->readChars && dIn->numReadChars != 0)) {
    setCallError(name, "null argument");
    return AwFmNullPtrError;
  }
  if (numReads >= (1ull << 32) || maxCandidates < 1 || maxCandidates > AWFM_CANDIDATES_MAX_SLOTS) {
    setCallError(name, "read numbers are 32-bit, and a read has 1 to 16 slots");
    return AwFmIllegalPositionError;
  }
  if (band > AWFM_VERIFY_MAX_BAND) {
    setCallError(name, "the band, maxDrift + 2 bandPad + 1 diagonals, holds 64 at the most");
    return AwFmIllegalPositionError;
  }
  return AwFmSuccess;
}

inline enum AwFmReturnCode scoringRefused(const char *name, const struct AwFmAlignScoring *scoring) {
  if (scoring->match < 1 || scoring->match > 255 || scoring->mismatch > 255 || scoring->gapOpen > 255 || scoring->gapExtend < 1 ||
      scoring->gapExtend > 255) {
    setCallError(name, "match and gapExtend are 1 to 255, mismatch and gapOpen 0 to 255");
    return AwFmIllegalPositionError;
  }
  return AwFmSuccess;
}

inline enum AwFmReturnCode matrixScoringRefused(const char *name, const struct AwFmMatrixScoring *scoring) {
  if (scoring->gapOpen > 255 || scoring->gapExtend < 1 || scoring->gapExtend > 255) {
    setCallError(name, "gapOpen is 0 to 255 and gapExtend 1 to 255");
    return AwFmIllegalPositionError;
  }
  return AwFmSuccess;
}

/* "end bonus": the matrix's ranges, then B */
inline enum AwFmReturnCode endBonusScoringRefused(const char *name, const struct AwFmMatrixScoring *scoring, const uint32_t endBonus) {
  const enum AwFmReturnCode rc = matrixScoringRefused(name, scoring);
  if (rc != AwFmSuccess) return rc;
  if (endBonus > AWFM_END_BONUS_MAX) {
    setCallError(name, "endBonus is 0 to 255");
    return AwFmIllegalPositionError;
  }
  return AwFmSuccess;
}

/* the caller holds image->recordMutex, and keeps it until after the launch: neither text nor record table is replaced before */
inline enum AwFmReturnCode textMissing(const char *name, const AwFmGpuImage *image) {
  if (image->dText) return AwFmSuccess;
  setCallError(name, "the image has no text (awfmGpuIndexSetText uploads it)");
  return AwFmUnsupportedVersionError;
}

/* the lanes of a group: the band's diagonals rounded up to 16, 32 or 64; $AWFM_GPU_DIAG `key` = 32 or 64 (tests) gives a group
 * more lanes than the band needs */
inline unsigned bandGroup(const uint64_t band, const char *key) {
  unsigned group = band <= 16u ? 16u : band <= 32u ? 32u : 64u;
  if (const char *env = awfmGpuDiag(key)) {
    const unsigned forced = (unsigned)atoi(env);
    if ((forced == 32u || forced == 64u) && forced > group) group = forced;
  }
  return group;
}

/* launches KERNEL<16>, <32> or <64> with the one argument p */
#define AWFM_LAUNCH_BAND_KERNEL(KERNEL, group, grid, block, stream, p)                                 \
  do {                                                                                                 \
    if ((group) == 16u) hipLaunchKernelGGL(KERNEL<16>, grid, block, 0, (hipStream_t)(stream), p);      \
    else if ((group) == 32u) hipLaunchKernelGGL(KERNEL<32>, grid, block, 0, (hipStream_t)(stream), p); \
    else hipLaunchKernelGGL(KERNEL<64>, grid, block, 0, (hipStream_t)(stream), p);                     \
  } while (0)

}  // namespace

#endif
