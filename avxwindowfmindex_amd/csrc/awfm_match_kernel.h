/*
 * awfm_match_kernel.h -- longest suffix match in batches (include/awfm_gpu.h: awfmGpuLongestSuffixMatches).
 *
 * For every query the kernel walks right to left like searchKernel (awfm_search_kernel.h) -- 4 lanes per query, one slice of a
 * block per lane, the query's characters in a 32-character register window, one query prefetched -- but it answers another
 * question: not "the range the stepping ends in" but "the last range that still had hits, and how many letters deep it is".
 *
 *   - every step produces a CANDIDATE range from the kept one; it is committed (and the match length grows) only when it is
 *     non-empty, and the walk ends at the first empty candidate or at the query's first character;
 *   - a table start is conditional: a non-empty entry of the last D letters (deeper table) or K letters (the index's own) IS
 *     r_D (r_K) and says that the match is at least that long; an empty entry says only that it is shorter -- the tables hold
 *     the first empty range, not the depth it appeared at -- and the walk starts from r_1;
 *   - a pair step (awfm_pair.h) covers two letters.  In its exact mode an empty pair range comes with the range after the first
 *     of the two letters out of the same registers: non-empty, it is committed as one more letter and the walk ends (the second
 *     letter is known to empty it); a flagged block leaves the range alone and the letter is stepped through the one-letter
 *     image;
 *   - when the walk crosses the left edge of the window, the window is re-filled with the 32 characters before it (the same
 *     aligned dword loads and v_alignbyte), so that fast steps and pair steps go on however long the match is;
 *   - the character loads of query i are aligned dwords between the one that holds its first walked byte and the one that
 *     holds ends[i] - 1 (later ones are clamped to that one): every dword read holds a byte of the query it is read for.
 *
 * Semantics: ref src/AwFmSearch.c:27-159 driven by a caller's loop (ref src/AwFmIndex.h:477-512); the host twin is
 * awfmLongestSuffixMatches (awfm_search_host.c).
 */
#ifndef AWFM_MATCH_KERNEL_H
#define AWFM_MATCH_KERNEL_H

#include "awfm_device.h"
#include "awfm_pair.h"

namespace {

constexpr int kMatchLanes = 4; /* lanes per query */

/* the 2-bit letter codes (character 0 of the window in bits 63..62) and the "not a,c,g,t,u" bits (bit i: character i) of a
 * group's 32-character window, lane `gl` holding characters 8 gl .. 8 gl + 7 in win[0..1]: the SWAR decode of searchKernel */
__device__ __forceinline__ void matchDecodeWindow(const unsigned (&win)[2], unsigned gl, unsigned long long &allCodes, unsigned &allBad) {
  unsigned long long codes = 0;
  unsigned bad = 0;
#pragma unroll
  for (int w = 0; w < 2; w++) {
    const unsigned word = win[w];
    unsigned t = (word >> 1) & 0x03030303u;
    t ^= (t >> 1) & 0x01010101u;
    const unsigned b0 = t & 0x01010101u, b1 = (t >> 1) & 0x01010101u, b01 = b0 & b1;
    const unsigned expect = 0x61616161u + (b0 << 1) + b1 * 6u + b01 * 11u; /* 'a','c','g','t' */
    unsigned diff = ((word | 0x20202020u) ^ expect) & ~b01;
    diff |= diff >> 4;
    diff |= diff >> 2;
    diff |= diff >> 1;
    diff &= 0x01010101u;
    const unsigned badBits = (diff & 1u) | ((diff >> 7) & 2u) | ((diff >> 14) & 4u) | ((diff >> 21) & 8u);
    const unsigned packed = ((t & 3u) << 6) | ((t >> 4) & 0x30u) | ((t >> 14) & 0x0Cu) | (t >> 24);
    codes = (codes << 8) | packed;
    bad |= badBits << (4 * w);
  }
  allCodes = groupSum64<kMatchLanes>(codes << (64 - 16 * ((int)gl + 1)));
  allBad = groupSum<kMatchLanes>(bad << (8 * gl));
}

/*
 * PAIR: nucleotide images with the pair image (two letters per block read where both are a,c,g,t/u inside the window).
 * starts == NULL: fixedLength characters per query.  Each of matchLengths / ranges / counts may be NULL.
 */
template <bool AMINO, bool NARROW, bool PAIR>
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(AMINO || (PAIR && !NARROW) ? 4 : 6, 8)))
    longestMatchKernel(const DevIndex ix, const unsigned char *__restrict__ chars, const unsigned long long *__restrict__ startsArg,
                       const unsigned long long *__restrict__ endsArg, const unsigned fixedLength, const unsigned long long numQueries,
                       const unsigned minLength, unsigned *__restrict__ matchLengthsArg, ulonglong2 *__restrict__ rangesArg,
                       unsigned *__restrict__ countsArg) {
  constexpr int G = kMatchLanes;
  constexpr int W = 8 / G;
  constexpr int kGroups = kThreads / G;
  typedef typename PositionType<NARROW>::type pos_t;
  static_assert(!PAIR || !AMINO, "pair steps: nucleotide");
  __shared__ unsigned long long sC[24];
  __shared__ unsigned sPow[32];
  __shared__ unsigned sPowDeep[AMINO ? 32 : 1];
  __shared__ AminoShared sAmino;
  __shared__ unsigned sMask[(kBlockMask + 1) * kSlices];
  __shared__ unsigned long long sSuper[!AMINO && !NARROW ? kMaxNucSuper * 4 : 1];
  __shared__ unsigned long long sPairC[PAIR ? 16 : 1];
  extern __shared__ unsigned sPairSuper[]; /* PAIR with ix.pairSuperInLds: the 16 pair bases of every superblock */
  if (PAIR) pairStageTables<NARROW, 16u>(ix, sPairC, sPairSuper);
  const unsigned card = AMINO ? 20u : 4u;
  if (threadIdx.x < 24) sC[threadIdx.x] = ix.prefixSums[threadIdx.x];
  stageMaskTable(sMask);
  if (!AMINO) nucStageSuper<NARROW>(ix, sSuper);
  if (AMINO && threadIdx.x < 32) { /* weight of table character j: 20^(k-1-j) (ref src/AwFmKmerTable.c:26-32) */
    unsigned w = 1, d = 1;
    for (unsigned e = threadIdx.x + 1; e < ix.seedK; e++) w *= card;
    for (unsigned e = threadIdx.x + 1; e < ix.deepK; e++) d *= card;
    sPow[threadIdx.x] = w;
    sPowDeep[threadIdx.x] = d;
  }
  if (AMINO) aminoStageTables(sAmino);
  __syncthreads();

  const unsigned gl = threadIdx.x % G; /* lane within the group = the block slice it holds */
  const unsigned firstWord = gl * W;   /* first of this lane's window dwords */
  const unsigned numGroups = gridDim.x * (unsigned)kGroups; /* (a persistent grid: at most CUs x 8 workgroups) */
  const unsigned long long groupId = ((unsigned long long)blockIdx.x * kThreads + threadIdx.x) / G;
  const unsigned charsMisalign = (unsigned)((unsigned long long)chars & 3ull);
  const unsigned char *charsAligned = chars - charsMisalign; /* stays a global-address-space pointer */
  const unsigned long long *starts = startsArg, *ends = endsArg;
  const bool listed = startsArg != nullptr; /* kernel argument: uniform */
  /* The kernel's uniform values (the image's view, the arguments, the loop's bounds) are more than the scalar registers hold
   * with the exec masks of the walk's nested branches; the ones read once per query live in vector registers instead, where
   * there is room (VEC_ARGS of them), so that nothing is spilled.  The counts are the smallest that leave no scalar spill with
   * the hipcc of ROCm 7 (found by raising them one at a time; tests/test_longest_match_resources.py pins the outcome -- no
   * spill, the planned vector registers -- so a compiler that allocates differently shows up there, and the cure is to raise
   * or lower these). */
  constexpr int VEC_ARGS = AMINO ? 5 : (PAIR ? 2 : 0);
  unsigned *matchLengths = matchLengthsArg;
  ulonglong2 *ranges = rangesArg;
  unsigned *counts = countsArg;
  if (VEC_ARGS >= 1) asm volatile("" : "+v"(matchLengths));
  if (VEC_ARGS >= 2) asm volatile("" : "+v"(ranges));
  if (VEC_ARGS >= 3) asm volatile("" : "+v"(counts));
  if (VEC_ARGS >= 4) asm volatile("" : "+v"(starts));
  if (VEC_ARGS >= 5) asm volatile("" : "+v"(ends));

  auto queryBounds = [&](unsigned long long q) -> ulonglong2 {
    if (listed) return make_ulonglong2(starts[q], ends[q]);
    return make_ulonglong2(q * fixedLength, q * fixedLength + fixedLength);
  };
  auto queryLength = [](const ulonglong2 &o) -> unsigned { /* of a query longer than 2^32 - 1 characters the last 2^32 - 1 */
    if (o.y <= o.x) return 0u;
    const unsigned long long d = o.y - o.x;
    return d > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned)d;
  };
  /* this lane's W + 1 aligned dwords of the window that begins at character wb of the query of `len` characters that ends
   * at byte `end` (len != 0); the address (+misalign) of the lane's first character comes back for the byte shift */
  auto requestWindow = [&](unsigned long long end, unsigned len, unsigned wb, unsigned (&raw)[W + 1]) -> unsigned {
    const unsigned long long mine = end - len + wb + 4u * firstWord + charsMisalign;
    const unsigned long long first = mine & ~3ull, last = (end - 1ull + charsMisalign) & ~3ull;
#pragma unroll
    for (int w = 0; w <= W; w++) {
      unsigned long long at = first + 4ull * w;
      at = at < last ? at : last;
      raw[w] = *(const unsigned *)(charsAligned + at);
    }
    return (unsigned)mine & 3u;
  };

  /* prefetched query: bounds and raw window dwords; listed: and the bounds of the query after it */
  ulonglong2 nOff = make_ulonglong2(0ull, 0ull), fOff = make_ulonglong2(0ull, 0ull);
  unsigned nRaw[W + 1];
  unsigned nShift = 0;
#pragma unroll
  for (int w = 0; w <= W; w++) nRaw[w] = 0u;
  unsigned long long q = groupId;
  if (q < numQueries) {
    nOff = queryBounds(q);
    const unsigned L = queryLength(nOff);
    if (L != 0u) nShift = requestWindow(nOff.y, L, L > 32u ? L - 32u : 0u, nRaw);
  }
  if (listed && q + numGroups < numQueries) fOff = queryBounds(q + numGroups);

  for (; q < numQueries; q += numGroups) {
    /* ---- the prefetched query becomes current ---- */
    const unsigned long long end = nOff.y;
    const unsigned len = queryLength(nOff);
    unsigned wb = len > 32u ? len - 32u : 0u; /* first character of the query inside the window */
    unsigned win[W];
#pragma unroll
    for (int w = 0; w < W; w++) win[w] = __builtin_amdgcn_alignbyte(nRaw[w + 1], nRaw[w], nShift);
    /* ---- prefetch the next query's window (listed: and the bounds of the one after) ---- */
    {
      const unsigned long long qn = q + numGroups;
      if (qn < numQueries) {
        nOff = listed ? fOff : queryBounds(qn);
        const unsigned L = queryLength(nOff);
        if (L != 0u) nShift = requestWindow(nOff.y, L, L > 32u ? L - 32u : 0u, nRaw);
      }
      if (listed && qn + numGroups < numQueries) fOff = queryBounds(qn + numGroups);
    }
    /* character i (wb <= i < wb + 32) of the query out of the register window */
    auto windowChar = [&](unsigned i) -> unsigned {
      const unsigned rel = i - wb;    /* 0..31 */
      const unsigned word = rel >> 2; /* 0..7: lane word / W, register word % W */
      unsigned lo = win[0], hi = win[W - 1]; /* named copies: a select over a two-element array becomes an indexed (scratch) load */
      asm volatile("" : "+v"(lo), "+v"(hi));
      const unsigned mine = (word & 1u) ? hi : lo;
      const unsigned v = groupShfl<G>(mine, word / W);
      return (v >> (8u * (rel & 3u))) & 0xFFu;
    };

    pos_t sp = 1, ep = 0;  /* the kept range: r_matched while matched != 0 */
    unsigned matched = 0;
    unsigned long long winCodes = 0;
    unsigned winBad = 0;
    bool alive = len != 0u;
    if (alive) {
      /* ---- conditional table start ---- */
      const unsigned e = len - wb; /* characters of the query inside the window: 1..32 */
      if (AMINO) {
        const unsigned K = ix.seedK, DK = ix.deepK;
        const bool trySeed = K != 0u && K <= 32u && len >= K, tryDeep = DK != 0u && DK <= 32u && len >= DK;
        unsigned partial = 0, partialDeep = 0, bad = 0; /* bad: bit 0 seed span, bit 1 deep span */
        if (trySeed || tryDeep) {
#pragma unroll
          for (int w = 0; w < W; w++) {
#pragma unroll
            for (unsigned b = 0; b < 4; b++) {
              const unsigned i = wb + 4u * (firstWord + w) + b; /* index in the query */
              const unsigned letter = aminoLetterIndex(sAmino, (win[w] >> (8u * b)) & 0xFFu);
              /* anything that is not one of the 20 letters has no table entry of its own (its index would carry into the next digit) */
              const bool inSeed = trySeed && i < len && i + K >= len, inDeep = tryDeep && i < len && i + DK >= len;
              partial += inSeed ? letter * sPow[(i + K - len) & 31u] : 0u;
              partialDeep += inDeep ? letter * sPowDeep[(i + DK - len) & 31u] : 0u;
              bad |= (inSeed && letter >= 20u ? 1u : 0u) | (inDeep && letter >= 20u ? 2u : 0u);
            }
          }
        }
        const unsigned index = groupSum<G>(partial), indexDeep = groupSum<G>(partialDeep);
        const unsigned flags = groupSum<G>((bad & 1u) | ((bad & 2u) << 7)); /* lanes with a bad seed span: bits 0..2, deep span: bits 8..10 */
        if (tryDeep && (flags >> 8) == 0u) {
          const ulonglong2 r = aminoDeepSeedEntry(ix, indexDeep);
          if (r.x <= r.y) {
            sp = (pos_t)r.x;
            ep = (pos_t)r.y;
            matched = DK;
          }
        }
        if (matched == 0u && trySeed && (flags & 0xFFu) == 0u && index < ix.seedLen) {
          const ulonglong2 r = ix.seed[index];
          if (r.x <= r.y) {
            sp = (pos_t)r.x;
            ep = (pos_t)r.y;
            matched = K;
          }
        }
      } else {
        matchDecodeWindow(win, gl, winCodes, winBad);
        /* (the depths through an opaque copy: the masks made of them are then computed here, per query, by a few scalar
         * instructions, instead of being hoisted out of the loop into scalar registers the kernel does not have) */
        unsigned dq = ix.deepK, kq = ix.seedK;
        asm volatile("" : "+s"(dq), "+s"(kq));
        const unsigned long long tail = e >= 32u ? winCodes : (winCodes >> (2u * (32u - e)));
        if (dq != 0u && dq < 32u && len >= dq && ((unsigned long long)winBad & (((1ull << dq) - 1ull) << (e - dq))) == 0ull) {
          const ulonglong2 r = deepSeedEntry(ix, tail & ((1ull << (2u * dq)) - 1ull));
          if (r.x <= r.y) {
            sp = (pos_t)r.x;
            ep = (pos_t)r.y;
            matched = dq;
          }
        }
        if (matched == 0u && kq != 0u && kq < 32u && len >= kq && ((unsigned long long)winBad & (((1ull << kq) - 1ull) << (e - kq))) == 0ull) {
          const unsigned long long index = tail & ((1ull << (2u * kq)) - 1ull);
          if (index < ix.seedLen) {
            const ulonglong2 r = ix.seed[index];
            if (r.x <= r.y) {
              sp = (pos_t)r.x;
              ep = (pos_t)r.y;
              matched = kq;
            }
          }
        }
      }
      if (matched == 0u) { /* r_1 (ref src/AwFmSearch.c:27-40); empty: a letter the text does not contain */
        const unsigned c = windowChar(len - 1u);
        const unsigned a = AMINO ? aminoLetterIndex(sAmino, c) : nucLetterIndex(c);
        const pos_t s1 = (pos_t)sC[a], e1 = (pos_t)(sC[a + 1] - 1ull);
        alive = s1 <= e1;
        if (alive) {
          sp = s1;
          ep = e1;
          matched = 1u;
        }
      }
    }

    /* ---- the walk: candidate steps from the kept range until one comes out empty ---- */
    while (alive && matched < len) {
      const unsigned pos = len - 1u - matched; /* the next character to the left */
      if (pos < wb) { /* (group-uniform) the walk crosses the window's left edge: the 32 characters before it */
        wb = wb > 32u ? wb - 32u : 0u;
        unsigned raw[W + 1];
        const unsigned shift = requestWindow(end, len, wb, raw);
#pragma unroll
        for (int w = 0; w < W; w++) win[w] = __builtin_amdgcn_alignbyte(raw[w + 1], raw[w], shift);
        if (!AMINO) matchDecodeWindow(win, gl, winCodes, winBad);
      }
      const unsigned r = pos - wb; /* 0..31 */
      pos_t csp = sp, cep = ep;
      unsigned extra = 0u; /* letters a non-empty candidate commits beyond the first */
      bool last = false;   /* the candidate is the final range */
      if (AMINO) {
        aminoStepAny<G, NARROW>(ix, sC, sAmino, sMask, gl, aminoLetterIndex(sAmino, windowChar(pos)), csp, cep);
      } else {
        const unsigned two = (unsigned)(winCodes >> (62u - 2u * r)) & 15u; /* codes of characters pos - 1 (bits 3..2) and pos (bits 1..0) */
        PairStep did = kPairFlagged;
        if (PAIR && r != 0u && ((winBad >> (r - 1u)) & 3u) == 0u) /* two characters, both a,c,g,t/u inside the window: one pair block */
          did = pairSearchStep<NARROW, true>(ix, sPairC, sPairSuper, sMask, gl, two, csp, cep, sC);
        if (PAIR && did != kPairFlagged) {
          /* stepped: csp/cep is the range after both letters, or the empty one after the first; died on the second: csp/cep is
           * the non-empty range after the first letter, which the second is known to empty */
          extra = did == kPairStepped ? 1u : 0u;
          last = did == kPairDiedOnSecond;
        } else if (((winBad >> r) & 1u) == 0u) { /* (a flagged pair block left csp/cep alone) */
          nucFastStep<G, NARROW>(ix, sC, sSuper, sMask, gl, two & 3u, csp, cep);
        } else {
          nucStepAny<G, NARROW>(ix, sC, sSuper, gl, nucLetterIndex(windowChar(pos)), csp, cep);
        }
      }
      alive = csp <= cep;
      if (alive) {
        sp = csp;
        ep = cep;
        matched += 1u + extra;
      }
      alive = alive && !last;
    }

    if (gl == 0) {
      const bool report = matched != 0u && matched >= minLength;
      if (matchLengths) matchLengths[q] = matched;
      if (ranges) ranges[q] = report ? make_ulonglong2((unsigned long long)sp, (unsigned long long)ep) : make_ulonglong2(1ull, 0ull);
      if (counts) counts[q] = report ? (unsigned)(ep - sp + (pos_t)1) : 0u;
    }
  }
}

}  // namespace

#endif
