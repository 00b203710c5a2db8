/*
 * awfm_window_affine_kernel.h -- scoreWindowsAffineKernel, the kernel of "window scores" (include/awfm_gpu.h): the full-width
 * local affine alignment of every read against the text window the caller names, with its begin and end cell and a chain slot.
 * The definition is the header's; the host twin and checker is awfm_window_affine.c.
 *
 * A WAVE PER READ over a persistent grid, as a systolic array: no scan and no trace.  LDS holds per wave the 64 read words and
 * the 64 boundary entries lane 0 is fed from, and the amino letter table.  Lane k owns Q consecutive columns of the window,
 * t = c0 + k Q + 1 .. c0 + k Q + Q, whose text letters it loads once as whole aligned dwords and keeps packed in Q / 4
 * registers.  Rows flow through the lanes a step apart: at step s lane k does row i = s - k + 1 for its Q columns, left to
 * right.  From lane k - 1 it takes that row's H and E of the column to its left, their origins and the row's read letter (above
 * the second origin's 26 bits): four moves by one lane per step, one DPP wave shift each.  It keeps last step's H and origin
 * for the diagonal.  H(i-1, .), F and their two origins stay in registers per column.  An origin is i << 13 | t in one word.
 * Lane 0's read letter comes from 64 aligned dwords of the read that the wave loads into LDS every 256 rows.
 *
 * Q is 4, 8 or 12, the smallest with 64 Q >= W, chosen per read (a wave-uniform switch; sixteen columns a lane do not fit the
 * register budget without spilling).  A window wider than 64 Q -- wider than 768 unless Q is forced -- goes in COLUMN BLOCKS of
 * 64 Q columns: lane 63 stores H, E and the two origins of its last column for every row (16 bytes) into the wave's arena in
 * the caller's scratch, lane 0 of the next block takes them back, 64 rows per load.  The arena has two halves that take turns,
 * and an agent-scope fence stands between a block's stores and the next block's loads.
 *
 * The end cell -- largest H, then smallest i, then smallest t -- is each lane's own best (strict-greater update, rows and columns
 * ascending) among the cells of two equal letters (DESIGN 4n proves that the end cell is one), and one butterfly over the wave on
 * H << 32 | ~i << 13 | ~t per block; one ballot finds the winner's lane and one read of that lane brings its origin.  EVERY
 * LOAD OF TEXT OR READ is an aligned dword that holds a byte the read or its clipped window owns, and the record is checked
 * against the text's length before anything is read.  Vector loads and stores only.
 */
#ifndef AWFM_WINDOW_AFFINE_KERNEL_H
#define AWFM_WINDOW_AFFINE_KERNEL_H

#include "awfm_band_kernel.h"

namespace {

constexpr unsigned kWinAffThreads = 256;     /* per workgroup: four waves, each with reads of its own */
constexpr unsigned kWinAffMaxVgprs = 128;    /* the budget of every instantiation: four waves per SIMD */
constexpr unsigned kWinAffBlocksPerCU = 4;   /* hence four workgroups of four waves per CU */
constexpr unsigned kWinAffLdsBytes = 5152;   /* per wave 64 boundary entries and 64 read words, and the amino letter table */
constexpr unsigned kWinAffMaxQ = 12;         /* columns per lane: 4, 8, 12 */
constexpr unsigned kWinAffEntryBytes = 16;   /* a row of a block's boundary column: H, E, O_H, O_E */
constexpr int kWinAffNeg = -0x40000000;      /* minus infinity: E and F are rebuilt from an H >= 0 in every cell, so it never drifts */
static_assert(AWFM_WINDOW_MAX_WIDTH < (1u << 13) && AWFM_WINDOW_MAX_LENGTH < (1u << 13), "an origin is 13 + 13 bits");

struct DevWindowParams {
  struct AwFmWindowInputs in;
  struct AwFmWindowOutputs out;
  const unsigned char *text;
  unsigned long long length;
  const unsigned long long *ends; /* the image's record table; numRecords == 0: one sequence [0, length) */
  unsigned numRecords;
  unsigned long long numReads;
  uint4 *arena;                   /* per wave of the grid 2 * maxLength entries */
  unsigned maxLength, stride, column, amino, floor, forcedQ; /* floor: max(minScore, 1); forcedQ: 0 or the Q of every read */
  int match, mismatch, open, extend;                        /* open: what the first character of a gap costs, o + e */
};

/* the launch's parameters where the launch left them, in the kernel's argument segment: a field is loaded where it is used
 * instead of living in a scalar register from the kernel's first instruction to its last (awfm_score_affine_kernel.h) */
typedef const __attribute__((address_space(4))) DevWindowParams *WindowParamsRef;

/* the value of the lane below, 0 in lane 0: DPP wave_shr:1 */
__device__ __forceinline__ unsigned winAffFromBelow(unsigned v) { return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xF, 0xF, true); }

/* R[0 .. n) against T[0 .. W), n and W >= 1: the key of the end cell, H << 32 | (0x1FFF - i) << 13 | (0x1FFF - t), and its origin;
 * every lane returns the same */
template <int Q>
__device__ __forceinline__ unsigned long long windowRead(const WindowParamsRef p, const unsigned char *R, const int n, const unsigned char *T,
                                                         const int W, uint4 *arena, const unsigned char *sAmino, unsigned *sRead,
                                                         uint4 *sBoundary, const unsigned lane, unsigned &origin) {
  constexpr int kBlockColumns = 64 * Q;
  const unsigned amino = p->amino, proper = amino ? 20u : 4u, maxLength = p->maxLength;
  const int match = p->match, mismatch = -p->mismatch, open = p->open, extend = p->extend;
  const unsigned readSkew = (unsigned)((unsigned long long)R & 3ull);
  const unsigned *readWords = (const unsigned *)(R - readSkew);
  unsigned long long bestKey = 0ull;
  origin = 0u;
#pragma nounroll
  for (int c0 = 0, block = 0; c0 < W; c0 += kBlockColumns, block++) {
    const int blockWidth = W - c0 < kBlockColumns ? W - c0 : kBlockColumns;
    const bool hasNext = c0 + kBlockColumns < W;
    const uint4 *arenaIn = arena + (size_t)(block & 1) * maxLength;
    uint4 *arenaOut = arena + (size_t)((block + 1) & 1) * maxLength;
    /* the lane's text: window characters [u0, u0 + Q), those below W */
    const int u0 = c0 + (int)lane * Q;
    const int valid = W - u0 < 0 ? 0 : W - u0 > Q ? Q : W - u0;
    unsigned letters[Q / 4];
    {
      const unsigned char *A = T + u0;
      const unsigned skew = (unsigned)((unsigned long long)A & 3ull);
      const unsigned *words = (const unsigned *)(A - skew);
      unsigned raw[Q / 4 + 1];
#pragma unroll
      for (int w = 0; w <= Q / 4; w++) {
        const int first = u0 - (int)skew + 4 * w; /* the window characters the word holds: [first, first + 4) */
        raw[w] = first < W && first + 4 > 0 && valid > 0 ? words[w] : 0u;
      }
#pragma unroll
      for (int w = 0; w < Q / 4; w++) {
        const unsigned four = (unsigned)((((unsigned long long)raw[w + 1] << 32) | raw[w]) >> (8u * skew));
        unsigned packed = 0u;
#pragma unroll
        for (int b = 0; b < 4; b++) {
          unsigned letter = verifyLetter(sAmino, amino, (four >> (8 * b)) & 0xFFu);
          letter = letter < proper && 4 * w + b < valid ? letter : 0xFFu; /* an ambiguity letter and a column beyond W match nothing */
          packed |= letter << (8 * b);
        }
        letters[w] = packed;
      }
    }
    int prevH[Q], prevF[Q];
    unsigned prevOH[Q], prevOF[Q];
#pragma unroll
    for (int j = 0; j < Q; j++) { /* row 0 */
      prevH[j] = 0;
      prevF[j] = kWinAffNeg;
      prevOH[j] = (unsigned)(u0 + j + 1);
      prevOF[j] = 0u;
    }
    int diagH = 0;
    unsigned diagO = (unsigned)u0; /* H(0, t - 1) of the lane's first column and its origin */
    int outH = 0, outE = kWinAffNeg;
    unsigned outOH = 0u, outOE = 0u; /* (outOE carries the row's read letter above the origin's 26 bits) */
    int bestH = 0;
    unsigned bestCell = 0u, bestO = 0u;
    const int lanesUsed = (blockWidth + Q - 1) / Q, steps = n + lanesUsed - 1;
#pragma nounroll
    for (int s = 0; s < steps; s++) {
      /* lane 0's row is s + 1: its read letter, and behind the first block its left neighbours from the arena */
      const unsigned at = readSkew + (unsigned)s;
      if (s == 0 || (at & 255u) == 0u) {
        const unsigned w = ((at >> 8) << 6) + lane;
        __builtin_amdgcn_wave_barrier(); /* (the steps before have read their words) */
        sRead[lane] = 4u * w < readSkew + (unsigned)n ? readWords[w] : 0u;
        __builtin_amdgcn_wave_barrier();
      }
      const unsigned fromRead = sRead[(at >> 2) & 63u];
      unsigned rowLetter = verifyLetter(sAmino, amino, (fromRead >> (8u * (at & 3u))) & 0xFFu);
      rowLetter = rowLetter < proper ? rowLetter : 0x3Fu;
      int leftH = (int)winAffFromBelow((unsigned)outH), leftE = (int)winAffFromBelow((unsigned)outE);
      unsigned leftOH = winAffFromBelow(outOH), leftOE = winAffFromBelow(outOE), letter = leftOE >> 26;
      leftOE &= 0x3FFFFFFu;
      if (block) {
        if ((s & 63) == 0) {
          const int row = s + (int)lane; /* entry `row` is row row + 1 */
          __builtin_amdgcn_wave_barrier();
          sBoundary[lane] = row < n ? arenaIn[row] : make_uint4(0u, 0u, 0u, 0u);
          __builtin_amdgcn_wave_barrier();
        }
        const uint4 boundary = sBoundary[s & 63];
        if (lane == 0u) {
          leftH = (int)boundary.x;
          leftE = (int)boundary.y;
          leftOH = boundary.z;
          leftOE = boundary.w;
        }
      } else if (lane == 0u) { /* column 0: H = 0 and its own origin, E = -inf */
        leftH = 0;
        leftE = kWinAffNeg;
        leftOH = (unsigned)(s + 1) << 13;
        leftOE = 0u;
      }
      letter = lane == 0u ? rowLetter : letter;
      const int i = s - (int)lane + 1;
      if (i >= 1 && i <= n) {
        int dH = diagH, hL = leftH, eL = leftE;
        unsigned dO = diagO, ohL = leftOH, oeL = leftOE;
        diagH = leftH;
        diagO = leftOH;
#pragma unroll
        for (int w = 0; w < Q / 4; w++) asm volatile("" : "+v"(letters[w])); /* (unpacked once per row, not once per block into Q registers) */
        const unsigned rowCell = ((unsigned)i << 13) + (unsigned)u0 + 1u; /* the origin of an H = 0 in the lane's first column */
#pragma unroll
        for (int j = 0; j < Q; j++) {
          const unsigned tLetter = (letters[j >> 2] >> (8 * (j & 3))) & 0xFFu;
          const bool same = tLetter == letter;
          const int M = dH + (same ? match : mismatch);
          const int fOpens = prevH[j] - open, fExtends = prevF[j] - extend;
          const bool fOpened = fOpens >= fExtends;
          const int F = fOpened ? fOpens : fExtends;
          const unsigned oF = fOpened ? prevOH[j] : prevOF[j];
          const int eOpens = hL - open, eExtends = eL - extend;
          const bool eOpened = eOpens >= eExtends;
          const int E = eOpened ? eOpens : eExtends;
          const unsigned oE = eOpened ? ohL : oeL;
          int H = M > F ? M : F;
          H = H > E ? H : E;
          H = H > 0 ? H : 0;
          unsigned oH = F == H ? oF : oE;
          oH = M == H ? dO : oH;
          oH = H == 0 ? rowCell + (unsigned)j : oH;
          /* strictly: the smallest i, then the smallest t of the lane's largest H.  Only a cell of two equal letters can be the end
           * cell: a gap leaves a larger H behind it, a mismatch one at least as large in an earlier row.  The columns
           * beyond W hold no letter and are left out with them */
          if (same && H > bestH) {
            bestH = H;
            bestCell = rowCell + (unsigned)j;
            bestO = oH;
          }
          dH = prevH[j];
          dO = prevOH[j];
          prevH[j] = H;
          prevOH[j] = oH;
          prevF[j] = F;
          prevOF[j] = oF;
          hL = H;
          eL = E;
          ohL = oH;
          oeL = oE;
        }
        outH = hL;
        outE = eL;
        outOH = ohL;
        outOE = oeL | (letter << 26);
        if (hasNext && lane == 63u) arenaOut[i - 1] = make_uint4((unsigned)hL, (unsigned)eL, ohL, oeL);
      }
    }
    /* the block's end cell: the largest H, then the smallest i, then the smallest t */
    const unsigned cellKey = ((0x1FFFu - (bestCell >> 13)) << 13) | (0x1FFFu - (bestCell & 0x1FFFu));
    const unsigned long long mine = ((unsigned long long)(unsigned)bestH << 32) | cellKey;
    unsigned long long key = mine;
#pragma unroll
    for (int step = 1; step < 64; step <<= 1) {
      const unsigned otherLow = (unsigned)__shfl_xor((int)(unsigned)key, step, 64), otherHigh = (unsigned)__shfl_xor((int)(unsigned)(key >> 32), step, 64);
      const unsigned long long other = ((unsigned long long)otherHigh << 32) | otherLow;
      key = other > key ? other : key;
    }
    const unsigned long long holders = __ballot(mine == key);
    const unsigned blockOrigin = (unsigned)__builtin_amdgcn_readlane((int)bestO, __ffsll((long long)holders) - 1);
    /* (every lane holds the key: into scalar registers) */
    key = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(key >> 32)) << 32) |
          (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)key);
    if (key > bestKey) {
      bestKey = key;
      origin = blockOrigin;
    }
    if (hasNext) __threadfence(); /* lane 63's stores of this block before lane 0's loads of the next */
  }
  return bestKey;
}

__global__ void __launch_bounds__(kWinAffThreads, 4) scoreWindowsAffineKernel(const DevWindowParams args) {
  (void)args;
  WindowParamsRef p = (WindowParamsRef)__builtin_amdgcn_kernarg_segment_ptr();
  __shared__ uint4 sBoundaryWords[kWinAffThreads / 64u][64];
  __shared__ unsigned sReadWords[kWinAffThreads / 64u][64];
  __shared__ unsigned char sAmino[32];
  uint4 *sBoundary = sBoundaryWords[threadIdx.x / 64u];
  unsigned *sRead = sReadWords[threadIdx.x / 64u];
  if (threadIdx.x < 32u) sAmino[threadIdx.x] = kAminoTables.letterOfAscii[threadIdx.x];
  __syncthreads();
  const unsigned lane = threadIdx.x & 63u;
  /* (read numbers are 32-bit, and so is the grid's number of waves) */
  const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kWinAffThreads / 64u) + threadIdx.x / 64u));
  const unsigned numWaves = gridDim.x * (kWinAffThreads / 64u);
  unsigned unscored = 0, found = 0;
  for (unsigned long long r = wave; r < p->numReads; r += numWaves) {
    asm volatile("" : "+s"(p)); /* (every trip takes the fields anew) */
    const unsigned s = p->in.windowSequences[r];
    unsigned value = AWFM_VERIFY_NONE, readBegin = 0u, readEnd = 0u;
    unsigned long long textBegin = 0ull, textEnd = 0ull;
    const bool looked = s != AWFM_CANDIDATES_NONE;
    if (looked) {
      value = AWFM_VERIFY_MALFORMED;
      const unsigned long long begin = p->in.windowBegins[r], end = p->in.windowEnds[r];
      const unsigned long long from = p->in.readOffsets[r], to = p->in.readOffsets[r + 1ull];
      bool ok = s < (p->numRecords ? p->numRecords : 1u) && begin <= end && from <= to && to <= p->in.numReadChars;
      unsigned long long S = 0ull, E = 0ull;
      if (ok) {
        S = p->numRecords && s ? p->ends[s - 1u] + 1ull : 0ull;
        E = p->numRecords ? p->ends[s] : p->length;
        ok = !(p->numRecords && s && S == 0ull) && E >= S && E <= p->length;
      }
      if (ok) {
        const unsigned long long L = E - S, b = begin < L ? begin : L, e = end < L ? end : L, W = e - b, n = to - from;
        const unsigned longest = p->maxLength < AWFM_WINDOW_MAX_LENGTH ? p->maxLength : AWFM_WINDOW_MAX_LENGTH;
        if (W > (unsigned long long)AWFM_WINDOW_MAX_WIDTH) {
          value = AWFM_VERIFY_TOO_WIDE;
        } else if (n > (unsigned long long)longest) {
          value = AWFM_VERIFY_TOO_LONG;
        } else if (n == 0ull || W == 0ull) {
          value = 0u; /* nothing is aligned, nothing is read */
        } else {
          const unsigned char *R = p->in.readChars + from, *T = p->text + S + b;
          const unsigned q = p->forcedQ ? p->forcedQ : W <= 256ull ? 4u : W <= 512ull ? 8u : 12u;
          uint4 *arena = p->arena + (unsigned long long)wave * 2ull * p->maxLength;
          unsigned origin;
          unsigned long long key;
          if (q == 4u) key = windowRead<4>(p, R, (int)n, T, (int)W, arena, sAmino, sRead, sBoundary, lane, origin);
          else if (q == 8u) key = windowRead<8>(p, R, (int)n, T, (int)W, arena, sAmino, sRead, sBoundary, lane, origin);
          else key = windowRead<12>(p, R, (int)n, T, (int)W, arena, sAmino, sRead, sBoundary, lane, origin);
          value = (unsigned)(key >> 32);
          if (value) {
            readEnd = 0x1FFFu - ((unsigned)(key >> 13) & 0x1FFFu);
            textEnd = b + (0x1FFFu - ((unsigned)key & 0x1FFFu));
            readBegin = origin >> 13;
            textBegin = b + (origin & 0x1FFFu);
          }
        }
      }
    }
    /* (every lane holds the read's values: the counters stay scalar) */
    const bool counts = looked && value < AWFM_VERIFY_TOO_LONG && value >= p->floor;
    unscored += looked && value >= AWFM_VERIFY_TOO_LONG ? 1u : 0u;
    found += counts ? 1u : 0u;
    if (lane == 0u) {
      if (p->out.scores) p->out.scores[r] = value;
      if (p->out.readBegins) p->out.readBegins[r] = readBegin;
      if (p->out.readEnds) p->out.readEnds[r] = readEnd;
      if (p->out.textBegins) p->out.textBegins[r] = textBegin;
      if (p->out.textEnds) p->out.textEnds[r] = textEnd;
      if (looked) {
        const unsigned long long at = r * p->stride + p->column;
        if (p->out.sequences) p->out.sequences[at] = counts ? s : AWFM_CANDIDATES_NONE;
        if (p->out.chainAnchors) p->out.chainAnchors[at] = counts ? 1u : 0u;
        if (p->out.chainReadBegins) p->out.chainReadBegins[at] = counts ? readBegin : 0u;
        if (p->out.chainReadEnds) p->out.chainReadEnds[at] = counts ? readEnd : 0u;
        if (p->out.chainBeginDiagonals) p->out.chainBeginDiagonals[at] = counts ? (long long)textBegin - (long long)readBegin : 0ll;
        if (p->out.chainEndDiagonals) p->out.chainEndDiagonals[at] = counts ? (long long)textEnd - (long long)readEnd : 0ll;
      }
    }
  }
  /* one atomic per wave and counter that met any */
  if (lane == 0u && unscored && p->out.numUnscored) atomicAdd((unsigned long long *)p->out.numUnscored, (unsigned long long)unscored);
  if (lane == 0u && found && p->out.numFound) atomicAdd((unsigned long long *)p->out.numFound, (unsigned long long)found);
}

}  // namespace

#endif
