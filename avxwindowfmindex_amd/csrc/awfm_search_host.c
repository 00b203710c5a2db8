/*
 * Host-side scalar primitives on the reference block layout.
 *
 * These serve (a) the index builder (seed-table fill) and (b) the single-query
 * entry points of AwFmIndex.h.  They are NOT used by awFmParallelSearchCount /
 * awFmParallelSearchLocate, which run on the GPU only (awfm_batch.c).
 */
#include <stdlib.h>
#include <string.h>
#include "awfm_internal.h"

static inline const uint8_t *blockAt(const struct AwFmIndex *ix, uint64_t block) {
  return (const uint8_t *)ix->bwtBlockList.asNucleotide + block * awfmBlockBytes(ix->config.alphabetType);
}

/* popcount of occVec(letter) over bits 0..p of one block
 * (ref src/AwFmOccurrence.c:8-135 + src/AwFmSimdConfig.c:89-114) */
static inline unsigned blockRank(const uint8_t *blk, unsigned planes, uint8_t ones, uint8_t zeros, unsigned p) {
  const uint64_t *w = (const uint64_t *)blk; /* plane j, word q at w[4*j + q] */
  unsigned total = 0;
  const unsigned last = p >> 6;
  for (unsigned q = 0; q <= last; q++) {
    uint64_t v = ~0ULL;
    for (unsigned j = 0; j < planes; j++) {
      const uint64_t plane = w[4 * j + q];
      const uint64_t wantOne = (uint64_t)0 - ((ones >> j) & 1u);
      const uint64_t wantZero = (uint64_t)0 - ((zeros >> j) & 1u);
      v &= (plane | ~wantOne) & (~plane | ~wantZero);
    }
    if (q == last) v &= ~0ULL >> (63 - (p & 63));
    total += (unsigned)__builtin_popcountll(v);
  }
  return total;
}

/* Occ(letter, q) (ref src/AwFmSearch.c:48-63) */
uint64_t awfmHostOcc(const struct AwFmIndex *ix, uint8_t letter, uint64_t q) {
  const bool amino = awfmIsAmino(ix);
  const unsigned planes = amino ? 5 : 3;
  const uint8_t *blk = blockAt(ix, q / AW_FM_POSITIONS_PER_FM_BLOCK);
  const uint64_t *base = (const uint64_t *)(blk + 32 * planes);
  const uint8_t ones = amino ? awfmAminoOnes[letter] : awfmNucOnes[letter];
  const uint8_t zeros = amino ? awfmAminoZeros[letter] : awfmNucZeros[letter];
  return base[letter] + blockRank(blk, planes, ones, zeros, (unsigned)(q % AW_FM_POSITIONS_PER_FM_BLOCK));
}

static void hostStep(const struct AwFmIndex *ix, struct AwFmSearchRange *range, uint8_t letter) {
  const uint64_t c = ix->prefixSums[letter];
  const uint64_t sp = c + awfmHostOcc(ix, letter, range->startPtr - 1);
  const uint64_t ep = c + awfmHostOcc(ix, letter, range->endPtr) - 1;
  range->startPtr = sp;
  range->endPtr = ep;
}

/* ref src/AwFmSearch.c:42-103 */
void awFmNucleotideIterativeStepBackwardSearch(const struct AwFmIndex *_RESTRICT_ const index,
                                               struct AwFmSearchRange *_RESTRICT_ const range,
                                               const uint8_t letterIndex) {
  hostStep(index, range, letterIndex);
}

/* ref src/AwFmSearch.c:105-159 */
void awFmAminoIterativeStepBackwardSearch(const struct AwFmIndex *_RESTRICT_ const index,
                                          struct AwFmSearchRange *_RESTRICT_ const range, const uint8_t letterIndex) {
  hostStep(index, range, letterIndex);
}

static inline uint8_t letterIndexOf(const struct AwFmIndex *ix, char c) {
  return awfmIsAmino(ix) ? awfmAminoAsciiToIndex((uint8_t)c) : awfmNucAsciiToIndex((uint8_t)c);
}

/* ref src/AwFmSearch.c:27-40 */
struct AwFmSearchRange awFmCreateInitialQueryRangeFromChar(const struct AwFmIndex *_RESTRICT_ const index,
                                                           const char letter) {
  const uint8_t a = letterIndexOf(index, letter);
  return (struct AwFmSearchRange){index->prefixSums[a], index->prefixSums[a + 1] - 1};
}

/* ref src/AwFmSearch.c:6-25 */
struct AwFmSearchRange awFmCreateInitialQueryRange(const struct AwFmIndex *_RESTRICT_ const index,
                                                   const char *_RESTRICT_ const query, const uint64_t queryLength) {
  return awFmCreateInitialQueryRangeFromChar(index, query[queryLength - 1]);
}

/* ref src/AwFmSearch.c:317-358 */
struct AwFmSearchRange awFmFindSearchRangeForString(const struct AwFmIndex *_RESTRICT_ const index,
                                                    const char *_RESTRICT_ const kmer, const size_t kmerLength) {
  size_t pos = kmerLength - 1;
  struct AwFmSearchRange range = awFmCreateInitialQueryRangeFromChar(index, kmer[pos]);
  while (range.startPtr <= range.endPtr && pos-- != 0) hostStep(index, &range, letterIndexOf(index, kmer[pos]));
  return range;
}

/* letter stored at a BWT position + LF step
 * (ref src/AwFmOccurrence.c:170-217, src/AwFmSearch.c:369-427); the sentinel maps to 0 */
uint64_t awfmHostLf(const struct AwFmIndex *ix, uint64_t p, uint8_t *letterOut) {
  const bool amino = awfmIsAmino(ix);
  const unsigned planes = amino ? 5 : 3;
  const uint8_t *blk = blockAt(ix, p / AW_FM_POSITIONS_PER_FM_BLOCK);
  const unsigned local = (unsigned)(p % AW_FM_POSITIONS_PER_FM_BLOCK);
  unsigned code = 0;
  for (unsigned j = 0; j < planes; j++) code |= ((blk[32 * j + local / 8] >> (local % 8)) & 1u) << j;
  const uint8_t letter = amino ? awfmAminoCodeToIndex((uint8_t)code) : awfmNucCodeToIndex((uint8_t)code);
  if (letterOut) *letterOut = letter;
  if (letter == (amino ? 21 : 5)) return 0;
  return ix->prefixSums[letter] + awfmHostOcc(ix, letter, p) - 1;
}

/* ref src/AwFmSearch.c:429-455; on the sentinel the position is left unchanged
 * and 0 is returned, as the reference does */
uint8_t awFmNucleotideBacktraceReturnPreviousLetterIndex(const struct AwFmIndex *_RESTRICT_ const index,
                                                         uint64_t *bwtPosition) {
  uint8_t letter;
  const uint64_t next = awfmHostLf(index, *bwtPosition, &letter);
  if (letter == 5) return 0;
  *bwtPosition = next;
  return letter;
}

/* ref src/AwFmSearch.c:457-483 */
uint8_t awFmAminoBacktraceReturnPreviousLetterIndex(const struct AwFmIndex *_RESTRICT_ const index,
                                                    uint64_t *bwtPosition) {
  uint8_t letter;
  const uint64_t next = awfmHostLf(index, *bwtPosition, &letter);
  if (letter == 21) return 0;
  *bwtPosition = next;
  return letter;
}

/* sampled SA value i, from memory or from the index file
 * (ref src/AwFmSuffixArray.c:149-177) */
static enum AwFmReturnCode sampledSaValue(const struct AwFmIndex *ix, uint64_t i, uint64_t *out) {
  if (ix->config.keepSuffixArrayInMemory && ix->suffixArray.values) {
    *out = awfmSaGet(ix->suffixArray.values, ix->suffixArray.valueBitWidth, i);
    return AwFmSuccess;
  }
  size_t v = 0;
  const enum AwFmReturnCode rc = awfmSaValueFromFile(ix, i, &v);
  *out = v;
  return rc;
}

/* ref src/AwFmSearch.c:248-282 */
uint64_t awFmFindDatabaseHitPositionSingle(const struct AwFmIndex *_RESTRICT_ const index,
                                           const uint64_t bwtPosition,
                                           enum AwFmReturnCode *_RESTRICT_ fileAccessResult) {
  const uint64_t ratio = index->config.suffixArrayCompressionRatio;
  uint64_t p = bwtPosition, offset = 0, value = 0;
  while (p % ratio != 0) {
    p = awfmHostLf(index, p, NULL);
    offset++;
  }
  if (sampledSaValue(index, p / ratio, &value) != AwFmSuccess) {
    *fileAccessResult = AwFmFileReadFail;
    return 0;
  }
  *fileAccessResult = AwFmFileReadOkay;
  return (value + offset) % index->bwtLength;
}

/* ref src/AwFmSearch.c:161-246: NULL + AwFmGeneralFailure for an empty range */
uint64_t *awFmFindDatabaseHitPositions(const struct AwFmIndex *_RESTRICT_ const index,
                                       const struct AwFmSearchRange *_RESTRICT_ const searchRange,
                                       enum AwFmReturnCode *_RESTRICT_ fileAccessResult) {
  const uint64_t hits = awFmSearchRangeLength(searchRange);
  if (hits == 0) {
    *fileAccessResult = AwFmGeneralFailure;
    return NULL;
  }
  uint64_t *positions = malloc(hits * sizeof(uint64_t));
  if (!positions) {
    *fileAccessResult = AwFmAllocationFailure;
    return NULL;
  }
  for (uint64_t i = 0; i < hits; i++) {
    enum AwFmReturnCode rc;
    positions[i] = awFmFindDatabaseHitPositionSingle(index, searchRange->startPtr + i, &rc);
    if (rc != AwFmFileReadOkay) {
      *fileAccessResult = AwFmFileReadFail;
      return positions;
    }
  }
  *fileAccessResult = AwFmFileReadOkay;
  return positions;
}

/* ---- longest suffix match (include/awfm_gpu.h: awfmLongestSuffixMatches) ----
 * The definition, letter by letter with the step above: no table enters it. */
struct awfmMatchCtx {
  const struct AwFmIndex *index;
  const uint8_t *chars;
  const uint64_t *starts, *ends;
  uint32_t fixedLength, minLength;
  uint32_t *matchLengths;
  struct AwFmSearchRange *ranges;
  uint32_t *counts;
};

static void awfmMatchRange(void *p, uint64_t begin, uint64_t end, unsigned tid) {
  (void)tid;
  const struct awfmMatchCtx *c = p;
  const struct AwFmIndex *ix = c->index;
  const uint32_t threshold = c->minLength > 1u ? c->minLength : 1u;
  for (uint64_t i = begin; i < end; i++) {
    const uint64_t first = c->starts ? c->starts[i] : i * c->fixedLength;
    const uint64_t last = c->starts ? c->ends[i] : first + c->fixedLength;
    uint64_t m = last > first ? last - first : 0;
    if (m > 0xFFFFFFFFull) m = 0xFFFFFFFFull; /* the match length is 32-bit: the last 2^32 - 1 characters */
    struct AwFmSearchRange kept = {1, 0};
    uint32_t length = 0;
    if (m != 0) {
      struct AwFmSearchRange r = awFmCreateInitialQueryRangeFromChar(ix, (char)c->chars[last - 1]);
      while (r.startPtr <= r.endPtr) {
        kept = r;
        length++;
        if (length == m) break;
        hostStep(ix, &r, letterIndexOf(ix, (char)c->chars[last - 1 - length]));
      }
    }
    if (length < threshold) kept = (struct AwFmSearchRange){1, 0};
    if (c->matchLengths) c->matchLengths[i] = length;
    if (c->ranges) c->ranges[i] = kept;
    if (c->counts) c->counts[i] = kept.startPtr <= kept.endPtr ? (uint32_t)(kept.endPtr - kept.startPtr + 1) : 0u;
  }
}

enum AwFmReturnCode awfmLongestSuffixMatches(const struct AwFmIndex *index, const uint8_t *chars, const uint64_t *starts,
                                             const uint64_t *ends, uint32_t fixedLength, uint64_t numQueries, uint32_t minLength,
                                             uint32_t *matchLengths, struct AwFmSearchRange *ranges, uint32_t *counts,
                                             unsigned threads) {
  if (!index) return AwFmNullPtrError;
  if (numQueries == 0) return AwFmSuccess;
  if (!chars || (starts == NULL) != (ends == NULL) || (!starts && fixedLength == 0)) return AwFmNullPtrError;
  struct awfmMatchCtx ctx = {index, chars, starts, ends, fixedLength, minLength, matchLengths, ranges, counts};
  awfmParallelFor(threads ? threads : 1, numQueries, awfmMatchRange, &ctx);
  return AwFmSuccess;
}

/* ---- one-substitution search (include/awfm_gpu.h: awfmOneSubstitutionSearch) ----
 * The definition, letter by letter with the step above: no table enters it.  Per query the ranges S_j = R(q[j..m)) of the
 * exact walk are kept; the variant (p, c) starts from one step of S_(p+1) with c (the initial range of c when p = m - 1) and
 * walks on over q[p-1] .. q[0].  Two passes over the batch: the first counts, the second -- after a prefix sum over the
 * counts -- stores the records of query i from slot first[i] on, which is the order by (query, edit). */
struct awfmSubstCtx {
  const struct AwFmIndex *index;
  const uint8_t *chars;
  const uint64_t *offsets;
  uint32_t fixedLength;
  int includeExact;
  uint32_t *hitQueries, *hitEdits;
  struct AwFmSearchRange *hitRanges;
  uint64_t capacity;
  uint64_t *first; /* numQueries + 1 words: pass 1 leaves the records of query i in first[i + 1] */
  uint32_t *variants;
  uint64_t *occurrences;
  int store;
  int failed;
};

static inline void awfmSubstEmit(const struct awfmSubstCtx *c, uint64_t slot, uint64_t query, uint32_t edit, struct AwFmSearchRange r) {
  if (!c->store || slot >= c->capacity) return;
  if (c->hitQueries) c->hitQueries[slot] = (uint32_t)query;
  if (c->hitEdits) c->hitEdits[slot] = edit;
  if (c->hitRanges) c->hitRanges[slot] = r;
}

static void awfmSubstRange(void *p, uint64_t begin, uint64_t end, unsigned tid) {
  (void)tid;
  struct awfmSubstCtx *c = p;
  const struct AwFmIndex *ix = c->index;
  const unsigned sigma = awfmIsAmino(ix) ? 20u : 4u;
  struct AwFmSearchRange *suffix = NULL; /* suffix[j] = S_j, j = live .. m - 1 */
  uint64_t room = 0;
  for (uint64_t i = begin; i < end; i++) {
    const uint64_t from = c->offsets ? c->offsets[i] : i * c->fixedLength;
    const uint64_t to = c->offsets ? c->offsets[i + 1] : from + c->fixedLength;
    uint64_t m = to > from ? to - from : 0;
    if (m > 0xFFFFFFFFull) m = 0; /* such a query has no records */
    const uint8_t *q = c->chars + from;
    uint64_t slot = c->store ? c->first[i] : 0, records = 0, occurrences = 0;
    if (m != 0) {
      if (m > room) {
        struct AwFmSearchRange *grown = realloc(suffix, m * sizeof *suffix);
        if (!grown) {
          __atomic_store_n(&c->failed, 1, __ATOMIC_RELAXED);
          break;
        }
        suffix = grown;
        room = m;
      }
      /* the exact walk: S_j for j = m - 1 down to `live`, the leftmost j with a non-empty S_j (m: none) */
      uint64_t live = m;
      struct AwFmSearchRange r = awFmCreateInitialQueryRangeFromChar(ix, (char)q[m - 1]);
      for (uint64_t j = m; j-- != 0;) {
        if (j != m - 1) hostStep(ix, &r, letterIndexOf(ix, (char)q[j]));
        if (r.startPtr > r.endPtr) break;
        suffix[j] = r;
        live = j;
      }
      /* variants in the order of their edits: p ascending, then c; S_(p+1) must be non-empty */
      const uint64_t firstP = live == m ? m - 1 : (live == 0 ? 0 : live - 1);
      for (uint64_t at = firstP; at < m && at < (1ull << 27); at++) {
        const uint8_t own = letterIndexOf(ix, (char)q[at]);
        for (unsigned letter = 0; letter < sigma; letter++) {
          if (letter == own) continue;
          struct AwFmSearchRange v;
          if (at == m - 1) {
            v = (struct AwFmSearchRange){ix->prefixSums[letter], ix->prefixSums[letter + 1] - 1};
          } else {
            v = suffix[at + 1];
            hostStep(ix, &v, (uint8_t)letter);
          }
          for (uint64_t j = at; v.startPtr <= v.endPtr && j-- != 0;) hostStep(ix, &v, letterIndexOf(ix, (char)q[j]));
          if (v.startPtr > v.endPtr) continue;
          awfmSubstEmit(c, slot + records, i, (uint32_t)(at * 32u + letter), v);
          records++;
          occurrences += v.endPtr - v.startPtr + 1;
        }
      }
      if (c->includeExact && live == 0) {
        awfmSubstEmit(c, slot + records, i, AWFM_EDIT_NONE, suffix[0]);
        records++;
        occurrences += suffix[0].endPtr - suffix[0].startPtr + 1;
      }
    }
    if (!c->store) {
      c->first[i + 1] = records;
      if (c->variants) c->variants[i] = (uint32_t)records;
      if (c->occurrences) c->occurrences[i] = occurrences;
    }
  }
  free(suffix);
}

enum AwFmReturnCode awfmOneSubstitutionSearch(const struct AwFmIndex *index, const uint8_t *chars, const uint64_t *offsets,
                                              uint32_t fixedLength, uint64_t numQueries, int includeExact, uint32_t *hitQueries,
                                              uint32_t *hitEdits, struct AwFmSearchRange *hitRanges, uint64_t capacity,
                                              uint64_t *numHits, uint32_t *variantsPerQuery, uint64_t *occurrencesPerQuery,
                                              unsigned threads) {
  if (!index) return AwFmNullPtrError;
  if (numQueries == 0) return AwFmSuccess;
  if (numQueries >= (1ull << 32)) return AwFmIllegalPositionError; /* query numbers are 32-bit */
  if (!chars || (!offsets && fixedLength == 0)) return AwFmNullPtrError;
  uint64_t *first = malloc((numQueries + 1) * sizeof *first);
  if (!first) return AwFmAllocationFailure;
  struct awfmSubstCtx ctx = {index, chars, offsets, fixedLength, includeExact, hitQueries, hitEdits, hitRanges, capacity,
                             first, variantsPerQuery, occurrencesPerQuery, 0, 0};
  awfmParallelFor(threads ? threads : 1, numQueries, awfmSubstRange, &ctx);
  if (__atomic_load_n(&ctx.failed, __ATOMIC_RELAXED)) { /* a worker ran out of memory: its counts are incomplete, nothing is reported */
    free(first);
    return AwFmAllocationFailure;
  }
  first[0] = 0;
  for (uint64_t i = 0; i < numQueries; i++) first[i + 1] += first[i];
  if (numHits) *numHits = first[numQueries];
  if (capacity != 0 && (hitQueries || hitEdits || hitRanges)) {
    ctx.store = 1;
    awfmParallelFor(threads ? threads : 1, numQueries, awfmSubstRange, &ctx);
  }
  free(first);
  return __atomic_load_n(&ctx.failed, __ATOMIC_RELAXED) ? AwFmAllocationFailure : AwFmSuccess;
}
