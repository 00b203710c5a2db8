/*
 * awfm_subst_kernel.h -- one-substitution search in batches (include/awfm_gpu.h: awfmGpuOneSubstitutionSearch).
 *
 * For every query q[0..m) the kernel reports the non-empty ranges of the strings at Hamming distance 1 (and, on request, of q
 * itself) without enumerating them.  4 lanes per query, one slice of a block per lane, as in searchKernel and longestMatchKernel.
 * The group walks q from the right keeping ONE range, S_(p+1) = R(q[p+1..m)), and at every position p it makes the candidate
 * ranges of the variants (p, c) -- then each candidate that is non-empty is walked left over q[p-1] .. q[0], letter by letter,
 * and appended when it survives.  An empty S_(p+1) ends the query: no variant left of it can occur.  Where the candidates come
 * from:
 *
 *   - TABLES, p inside the last D letters (D = the deeper table's depth, or the K of the index's own table, when the query has
 *     that many letters and all of them are a,c,g,t/u): the entry of the D-mer with letter p replaced IS the variant's range
 *     after D letters (the tables hold the range the letter-by-letter stepping reaches, or the first empty one).  Lane c gathers
 *     the entry of letter c: one load instruction per position, four entries.  The lane whose letter is q[p]'s own reads the
 *     unedited entry, which is S_(m-D): the exact walk starts there.
 *   - nucleotide, left of that span or without a table: nucStepAllLetters (awfm_device.h) -- one pair of block reads, every lane
 *     counts the four letters on its slice, lane c leaves with the range of letter c.  The range of q[p]'s own letter is S_p.
 *   - amino: one aminoStepAny per letter (21 rounds per position: the 20 proper letters, and q[p]'s own when it is none of them).
 *   - p = m - 1: the initial ranges {C[c], C[c + 1] - 1}.
 *
 * The walk of the candidates is ONE piece of code behind all of these (a 4-bit mask of lanes that hold a candidate).  Records
 * are appended per wave instruction (sparseAppend's pattern: ballot, one returning atomic of the leader, vector stores) through
 * a 64-bit counter, bounded by the capacity; the per-query record and occurrence counts are plain stores.
 *
 * Characters: dword loads at aligned addresses between the one that holds the query's first byte and the one that holds its
 * last: every dword read holds a byte of the query it is read for.
 *
 * Semantics: ref src/AwFmSearch.c:27-159, :317-358; the host twin is awfmOneSubstitutionSearch (awfm_search_host.c).
 */
#ifndef AWFM_SUBST_KERNEL_H
#define AWFM_SUBST_KERNEL_H

#include "awfm_device.h"

namespace {

constexpr int kSubstLanes = 4;              /* lanes per query */
constexpr unsigned kSubstMaxPosition = 1u << 27; /* positions from here on are not substituted: edit = p * 32 + c is 32-bit */

struct SubstOut {
  unsigned *queries;
  unsigned *edits;
  ulonglong2 *ranges;
  unsigned long long capacity;
  unsigned long long *count;      /* NULL: nothing is appended */
  unsigned *variants;             /* per query, may be NULL */
  unsigned long long *occurrences; /* per query, may be NULL */
};

/* the lists up to their capacity as "no record": {0xFFFFFFFF, 0xFFFFFFFF, {1, 0}}; the counter to 0 */
__global__ void __launch_bounds__(256) oneSubstitutionFillKernel(const SubstOut out) {
  const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
  for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < out.capacity; i += stride) {
    if (out.queries) out.queries[i] = 0xFFFFFFFFu;
    if (out.edits) out.edits[i] = 0xFFFFFFFFu;
    if (out.ranges) out.ranges[i] = make_ulonglong2(1ull, 0ull);
  }
  if (out.count && blockIdx.x == 0 && threadIdx.x == 0) *out.count = 0ull;
}

__device__ __forceinline__ void substAppend(const SubstOut &out, bool hit, unsigned query, unsigned edit, unsigned long long sp,
                                            unsigned long long ep) {
  if (!out.count) return; /* kernel argument: uniform */
  const unsigned long long mask = __ballot(hit);
  if (mask == 0ull) return; /* uniform over the lanes that are here */
  const unsigned lane = threadIdx.x & 63u;
  const int leader = __ffsll((long long)mask) - 1;
  unsigned long long base = 0;
  if ((int)lane == leader) base = atomicAdd(out.count, (unsigned long long)__popcll(mask));
  base = ((unsigned long long)(unsigned)__shfl((int)(unsigned)(base >> 32), leader, 64) << 32) | (unsigned)__shfl((int)(unsigned)base, leader, 64);
  if (hit) {
    const unsigned long long slot = base + (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
    if (slot < out.capacity) {
      if (out.queries) out.queries[slot] = query;
      if (out.edits) out.edits[slot] = edit;
      if (out.ranges) out.ranges[slot] = make_ulonglong2(sp, ep);
    }
  }
}

__device__ __forceinline__ unsigned substShfl(unsigned v, unsigned from) { return groupShfl<kSubstLanes>(v, from); }
__device__ __forceinline__ unsigned long long substShfl(unsigned long long v, unsigned from) {
  return ((unsigned long long)groupShfl<kSubstLanes>((unsigned)(v >> 32), from) << 32) | groupShfl<kSubstLanes>((unsigned)v, from);
}

/*
 * TABLES: nucleotide, candidates inside the span of the deeper table / the index's own from gathers (see above); without it
 * the kernel is the definition letter by letter (the call's plain path).  offsets == NULL: fixedLength characters per query.
 */
template <bool AMINO, bool NARROW, bool TABLES>
__global__ void __launch_bounds__(kThreads)
    oneSubstitutionKernel(const DevIndex ix, const unsigned char *__restrict__ chars, const unsigned long long *__restrict__ offsetsArg,
                          const unsigned fixedLength, const unsigned long long numQueriesArg, const unsigned includeExact,
                          const SubstOut outArg) {
  constexpr int G = kSubstLanes;
  constexpr int kGroups = kThreads / G;
  typedef typename PositionType<NARROW>::type pos_t;
  static_assert(!(AMINO && TABLES), "table gathers: nucleotide");
  __shared__ unsigned long long sC[24];
  __shared__ AminoShared sAmino;
  __shared__ unsigned sMask[(kBlockMask + 1) * kSlices];
  __shared__ unsigned long long sSuper[!AMINO && !NARROW ? kMaxNucSuper * 4 : 1];
  if (threadIdx.x < 24) sC[threadIdx.x] = ix.prefixSums[threadIdx.x];
  stageMaskTable(sMask);
  if (!AMINO) nucStageSuper<NARROW>(ix, sSuper);
  if (AMINO) aminoStageTables(sAmino);
  __syncthreads();

  const unsigned gl = threadIdx.x % G; /* lane within the group = the block slice it holds = (nucleotide) the letter it branches with */
  unsigned long long numGroups = (unsigned long long)gridDim.x * kGroups;
  const unsigned long long groupId = ((unsigned long long)blockIdx.x * kThreads + threadIdx.x) / G;
  const unsigned charsMisalign = (unsigned)((unsigned long long)chars & 3ull);
  const unsigned char *charsAligned = chars - charsMisalign; /* stays a global-address-space pointer */
  /* TABLES: the kernel's uniform values are more than the scalar registers hold beside the exec masks of its nested branches;
   * the ones read once per query, per record or per gather live in vector registers instead, where there is room, so that
   * nothing is spilled (longestMatchKernel does the same; tests/test_one_substitution_resources.py pins the outcome). */
  SubstOut out = outArg;
  DevIndex tx = ix; /* the view the table gathers read */
  const unsigned long long *offsets = offsetsArg;
  unsigned long long numQueries = numQueriesArg;
  const bool listed = offsetsArg != nullptr; /* kernel argument: uniform */
  if (TABLES) {
    asm volatile("" : "+v"(out.queries), "+v"(out.edits), "+v"(out.ranges), "+v"(out.capacity));
    asm volatile("" : "+v"(out.variants), "+v"(out.occurrences), "+v"(offsets));
    asm volatile("" : "+v"(tx.deepSeed), "+v"(tx.deepBigBySp), "+v"(tx.seed));
    asm volatile("" : "+v"(charsAligned), "+v"(numGroups));
    if (!NARROW) asm volatile("" : "+v"(numQueries));
  }

  for (unsigned long long q = groupId; q < numQueries; q += numGroups) {
    const unsigned long long from = listed ? offsets[q] : q * fixedLength;
    const unsigned long long to = listed ? offsets[q + 1] : from + fixedLength;
    const unsigned len = to > from && to - from <= 0xFFFFFFFFull ? (unsigned)(to - from) : 0u;
    const unsigned long long base = from + charsMisalign;
    /* character i of the query, out of the aligned dword that holds it */
    auto charAt = [&](unsigned i) -> unsigned {
      const unsigned long long at = base + i;
      const unsigned word = *(const unsigned *)(charsAligned + (at & ~3ull));
      return (word >> (8u * ((unsigned)at & 3u))) & 0xFFu;
    };
    auto stepLetter = [&](unsigned c, pos_t &a, pos_t &b) {
      if (AMINO) {
        aminoStepAny<G, NARROW>(ix, sC, sAmino, sMask, gl, aminoLetterIndex(sAmino, c), a, b);
      } else {
        const unsigned letter = nucLetterIndex(c);
        if (letter < 4u) nucFastStep<G, NARROW>(ix, sC, sSuper, sMask, gl, letter, a, b);
        else nucStepAny<G, NARROW>(ix, sC, sSuper, gl, letter, a, b);
      }
    };

    unsigned records = 0;
    unsigned long long occurrences = 0;
    pos_t sp = 1, ep = 0;    /* S_p once position p has been handled */
    bool alive = len != 0u;  /* S_p is non-empty (or nothing has been stepped yet) */
    unsigned p = len;        /* positions p .. len - 1 have been handled */
    unsigned tabDepth = 0, tabLeft = 0; /* TABLES: depth of the table in use, positions of its span still to branch at */
    bool tabDeep = false;
    unsigned long long tail = 0;        /* TABLES: 2-bit codes of the last tabDepth letters, the last one in bits 1..0 */
    unsigned round = 0;                 /* amino: the letter the next round tries (20: the query's own, when it is not proper) */
    pos_t nextSp = 1, nextEp = 0;       /* amino: S_(p-1) while the rounds of position p - 1 run */

    if (TABLES && len != 0u) {
      auto spanCodes = [&](unsigned d, unsigned long long &codes) -> bool { /* false: a letter that is not a,c,g,t/u */
        unsigned bad = 0;
        codes = 0;
        for (unsigned j = 0; j < d; j++) {
          const unsigned c = charAt(len - d + j);
          const unsigned y = (c >> 1) & 3u;
          codes = (codes << 2) | (y ^ (y >> 1));
          bad |= nucIsAcgtu(c) ^ 1u;
        }
        return (bad & 1u) == 0u;
      };
      unsigned d = ix.deepK;
      if (d != 0u && d < 32u && len >= d && spanCodes(d, tail)) {
        tabDepth = d;
        tabDeep = true;
      } else {
        d = ix.seedK;
        if (d != 0u && d < 32u && len >= d && spanCodes(d, tail)) tabDepth = d; /* (a span of a,c,g,t/u: an index below 4^d, the table's length) */
      }
      tabLeft = tabDepth;
    }

    for (;;) {
      /* ---- the candidates of one position (amino: of one letter at one position) ---- */
      unsigned candMask = 0; /* lanes that hold a non-empty candidate; lane k's letter is firstLetter + k */
      pos_t csp = 1, cep = 0;
      unsigned position = 0, firstLetter = 0;
      unsigned left = 0; /* characters of the query to the left of what the candidate covers */
      if (TABLES && tabLeft != 0u) {
        const unsigned j = tabDepth - tabLeft; /* the span's letters from the right */
        tabLeft--;
        position = len - 1u - j;
        left = len - tabDepth;
        const unsigned own = (unsigned)(tail >> (2u * j)) & 3u;
        const unsigned long long index = tail ^ ((unsigned long long)(own ^ gl) << (2u * j));
        ulonglong2 r = make_ulonglong2(1ull, 0ull);
        if (tabDeep) r = deepSeedEntry(tx, index);
        else r = tx.seed[index];
        csp = (pos_t)r.x;
        cep = (pos_t)r.y;
        if (j == 0u) { /* the lane of the letter's own code read the unedited entry: S_(len - tabDepth) */
          sp = substShfl(csp, own);
          ep = substShfl(cep, own);
          alive = sp <= ep;
          p = left;
        }
        candMask = groupSum<G>(gl != own && r.x <= r.y ? 1u << gl : 0u);
      } else if (p == 0u || !alive) {
        break;
      } else if (AMINO) {
        position = p - 1u;
        left = position;
        const unsigned own = aminoLetterIndex(sAmino, charAt(position));
        const unsigned letter = round < 20u ? round : own;
        if (round < 20u || own >= 20u) {
          if (position == len - 1u) {
            csp = (pos_t)sC[letter];
            cep = (pos_t)(sC[letter + 1u] - 1ull);
          } else {
            csp = sp;
            cep = ep;
            aminoStepAny<G, NARROW>(ix, sC, sAmino, sMask, gl, letter, csp, cep);
          }
          if (letter == own) {
            nextSp = csp;
            nextEp = cep;
          } else if (csp <= cep) {
            candMask = 1u;
            firstLetter = round;
          }
        }
        if (++round == 21u) {
          round = 0u;
          sp = nextSp;
          ep = nextEp;
          alive = sp <= ep;
          p = position;
        }
      } else {
        position = p - 1u;
        left = position;
        const unsigned own = nucLetterIndex(charAt(position));
        pos_t ownSp, ownEp;
        if (position == len - 1u) {
          csp = (pos_t)sC[gl];
          cep = (pos_t)(sC[gl + 1u] - 1ull);
          ownSp = (pos_t)sC[own];
          ownEp = (pos_t)(sC[own + 1u] - 1ull);
        } else {
          nucStepAllLetters<NARROW>(ix, sC, sSuper, sMask, gl, sp, ep, csp, cep);
          ownSp = sp;
          ownEp = ep;
          if (own >= 4u) nucStepAny<G, NARROW>(ix, sC, sSuper, gl, own, ownSp, ownEp); /* (group-uniform) */
        }
        if (own < 4u) {
          ownSp = substShfl(csp, own);
          ownEp = substShfl(cep, own);
        }
        candMask = groupSum<G>(gl != own && csp <= cep ? 1u << gl : 0u);
        sp = ownSp;
        ep = ownEp;
        alive = sp <= ep;
        p = position;
      }
      /* (only a query of more than 2^27 characters gets here with such a position: its candidates were still computed above --
       * amino all 21 rounds, nucleotide the all-letters step, which the exact walk needs anyway -- and are dropped here) */
      if (position >= kSubstMaxPosition) candMask = 0u;

      /* ---- every candidate is walked to the query's first character, by the whole group ---- */
      for (unsigned k = 0; k < (AMINO ? 1u : 4u); k++) {
        if (((candMask >> k) & 1u) == 0u) continue; /* (group-uniform) */
        pos_t bsp = substShfl(csp, k), bep = substShfl(cep, k);
        unsigned at = left;
        while (at != 0u && bsp <= bep) {
          at--;
          stepLetter(charAt(at), bsp, bep);
        }
        const bool hit = bsp <= bep;
        if (hit) {
          records++;
          occurrences += (unsigned long long)(bep - bsp) + 1ull;
        }
        substAppend(out, hit && gl == 0u, (unsigned)q, position * 32u + firstLetter + k, (unsigned long long)bsp, (unsigned long long)bep);
      }
    }

    const bool exact = includeExact != 0u && len != 0u && alive && p == 0u;
    if (exact) {
      records++;
      occurrences += (unsigned long long)(ep - sp) + 1ull;
    }
    substAppend(out, exact && gl == 0u, (unsigned)q, 0xFFFFFFFFu, (unsigned long long)sp, (unsigned long long)ep);
    if (gl == 0u) {
      if (out.variants) out.variants[q] = records;
      if (out.occurrences) out.occurrences[q] = occurrences;
    }
  }
}

}  // namespace

#endif
