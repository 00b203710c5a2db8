/*
 * awfm_strings.c -- awfmAlignmentStrings (include/awfm_gpu.h, "alignment strings"): the CIGAR and the MD:Z string of every aligned
 * read, packed.  The host twin of awfmGpuAlignmentStrings and its checker: a read at a time, the header's rules as written.  ONE
 * formatter both counts and writes (dst == NULL: count), so a length and the bytes behind it cannot disagree.  Three passes: the
 * lengths over `threads` threads, the prefix sums on one, the bytes over `threads` threads.  Exact and readable rather than
 * fast.  The reference has no analogue (it stops at positions: ref src/AwFmParallelSearch.c:315-365).
 */
#include <stdlib.h>
#include <string.h>

#include "awfm_gpu.h"
#include "awfm_internal.h"

#define AWFM_STRINGS_MAX_TEXT (2ull * AWFM_ALIGN_MAX_LENGTH)

/* `value` in decimal without leading zeros at dst + at (dst == NULL: nothing is stored); returns where it ends */
static uint64_t awfmStringsDecimal(uint8_t *dst, uint64_t at, uint64_t value) {
  unsigned digits = 1;
  for (uint64_t v = value; v >= 10u; v /= 10u) digits++;
  if (dst) {
    uint64_t v = value;
    for (unsigned d = digits; d > 0; d--, v /= 10u) dst[at + d - 1u] = (uint8_t)('0' + v % 10u);
  }
  return at + digits;
}

static uint64_t awfmStringsByte(uint8_t *dst, uint64_t at, uint8_t c) {
  if (dst) dst[at] = c;
  return at + 1u;
}

static uint8_t awfmStringsLetter(uint8_t c, int amino) {
  if (c >= 'a' && c <= 'z') return (uint8_t)(c - 'a' + 'A');
  if (c >= 'A' && c <= 'Z') return c;
  return amino ? 'X' : 'N';
}

static int awfmStringsOpIsLegal(uint32_t op) { return op == 1u || op == 2u || op == AWFM_ALIGN_OP_S || op == 7u || op == 8u; }

/* the read and the text length of a row of k runs; 0 when a run has no length or no legal operation */
static int awfmStringsRowLengths(const uint32_t *row, uint32_t k, uint64_t *readLength, uint64_t *textLength) {
  uint64_t rn = 0, tn = 0;
  for (uint32_t i = 0; i < k; i++) {
    const uint64_t len = row[i] >> 4;
    const uint32_t op = row[i] & 15u;
    if (len == 0 || !awfmStringsOpIsLegal(op)) return 0;
    if (op != 2u) rn += len;
    if (op == 2u || op >= 7u) tn += len;
  }
  *readLength = rn;
  *textLength = tn;
  return 1;
}

/* the CIGAR of a checked row; classic: runs of '=' and 'X' next to each other are one M */
static uint64_t awfmStringsCigar(const uint32_t *row, uint32_t k, int classic, uint8_t *dst) {
  static const char letters[9] = {0, 'I', 'D', 0, 'S', 0, 0, '=', 'X'};
  uint64_t at = 0, merged = 0;
  for (uint32_t i = 0; i < k; i++) {
    const uint64_t len = row[i] >> 4;
    const uint32_t op = row[i] & 15u;
    if (classic && op >= 7u) {
      merged += len;
      const int goesOn = i + 1u < k && (row[i + 1u] & 15u) >= 7u;
      if (!goesOn) {
        at = awfmStringsByte(dst, awfmStringsDecimal(dst, at, merged), 'M');
        merged = 0;
      }
      continue;
    }
    at = awfmStringsByte(dst, awfmStringsDecimal(dst, at, len), (uint8_t)letters[op]);
  }
  return at;
}

/* the MD of a checked row whose text begins at `text` + p; the text is read only when dst is given */
static uint64_t awfmStringsMd(const uint32_t *row, uint32_t k, const uint8_t *text, uint64_t p, int amino, uint8_t *dst) {
  uint64_t at = 0, m = 0;
  for (uint32_t i = 0; i < k; i++) {
    const uint64_t len = row[i] >> 4;
    const uint32_t op = row[i] & 15u;
    if (op == 7u) {
      m += len;
      p += len;
    } else if (op == 8u) {
      for (uint64_t c = 0; c < len; c++, p++) {
        at = awfmStringsByte(dst, awfmStringsDecimal(dst, at, m), dst ? awfmStringsLetter(text[p], amino) : 0);
        m = 0;
      }
    } else if (op == 2u) {
      at = awfmStringsByte(dst, awfmStringsDecimal(dst, at, m), '^');
      for (uint64_t c = 0; c < len; c++, p++) at = awfmStringsByte(dst, at, dst ? awfmStringsLetter(text[p], amino) : 0);
      m = 0;
    }
  }
  return awfmStringsDecimal(dst, at, m);
}

struct awfmStringsCtx {
  const struct AwFmStringInputs *in;
  const struct AwFmStringOutputs *out;
  const uint8_t *text;
  const uint64_t *ends;
  uint64_t length, numRecords;
  uint32_t slots, maxOps;
  int classic, amino;
  uint32_t *cigarLengths, *mdLengths; /* [numReads]; 0 and 0: NONE or SKIPPED */
  uint64_t *textAt;                   /* [numReads]  global position of the script's first text character */
  uint64_t skipped[64], overflow[64]; /* per thread of the loop */
};

/* SKIPPED or not, by the header's list; *p: where the script's text begins */
static int awfmStringsReadIsGood(const struct awfmStringsCtx *c, uint64_t r, uint32_t k, uint64_t *p) {
  if (k > c->maxOps) return 0;
  const uint32_t j = c->in->slots[r];
  if (j >= c->slots) return 0;
  const uint32_t s = c->in->sequences[r * c->slots + j];
  if (s >= (c->numRecords ? c->numRecords : 1u)) return 0;
  const uint64_t S = c->numRecords && s ? c->ends[s - 1u] + 1u : 0u, E = c->numRecords ? c->ends[s] : c->length;
  if ((c->numRecords && s && S == 0) || E < S || E > c->length) return 0;
  uint64_t rn, tn;
  if (!awfmStringsRowLengths(c->in->ops + r * c->maxOps, k, &rn, &tn)) return 0;
  if (rn > AWFM_ALIGN_MAX_LENGTH || tn > AWFM_STRINGS_MAX_TEXT) return 0;
  const uint64_t L = E - S, tb = c->in->textBegins[r];
  if (tb > L || tn > L - tb) return 0;
  *p = S + tb;
  return 1;
}

static void awfmStringsLengthsRange(void *ctx, uint64_t begin, uint64_t end, unsigned tid) {
  struct awfmStringsCtx *c = ctx;
  uint64_t skipped = 0;
  for (uint64_t r = begin; r < end; r++) {
    const uint32_t k = c->in->numOps[r];
    c->cigarLengths[r] = c->mdLengths[r] = 0;
    if (k == 0) continue;
    if (!awfmStringsReadIsGood(c, r, k, &c->textAt[r])) {
      skipped++;
      continue;
    }
    const uint32_t *row = c->in->ops + r * c->maxOps;
    c->cigarLengths[r] = (uint32_t)awfmStringsCigar(row, k, c->classic, NULL);
    c->mdLengths[r] = (uint32_t)awfmStringsMd(row, k, NULL, 0, c->amino, NULL);
  }
  c->skipped[tid & 63u] += skipped;
}

static void awfmStringsWriteRange(void *ctx, uint64_t begin, uint64_t end, unsigned tid) {
  struct awfmStringsCtx *c = ctx;
  const struct AwFmStringOutputs *out = c->out;
  uint64_t overflow = 0;
  for (uint64_t r = begin; r < end; r++) {
    if (c->cigarLengths[r] == 0) continue; /* (a read with strings has a run, hence a CIGAR) */
    const uint32_t *row = c->in->ops + r * c->maxOps;
    const uint32_t k = c->in->numOps[r];
    int missed = 0;
    if (out->cigarChars) {
      if (out->cigarOffsets[r + 1u] <= out->cigarCapacity) awfmStringsCigar(row, k, c->classic, out->cigarChars + out->cigarOffsets[r]);
      else missed = 1;
    }
    if (out->mdChars) {
      if (out->mdOffsets[r + 1u] <= out->mdCapacity) awfmStringsMd(row, k, c->text, c->textAt[r], c->amino, out->mdChars + out->mdOffsets[r]);
      else missed = 1;
    }
    overflow += (uint64_t)missed;
  }
  c->overflow[tid & 63u] += overflow;
}

enum AwFmReturnCode awfmAlignmentStrings(const struct AwFmStringInputs *in, uint64_t numReads, uint32_t maxCandidates, uint32_t maxOps,
                                         uint32_t flags, const uint8_t *text, uint64_t length, const uint64_t *sequenceEnds,
                                         uint64_t numRecords, enum AwFmAlphabetType alphabet, const struct AwFmStringOutputs *out,
                                         unsigned threads) {
  if (numReads == 0) return AwFmSuccess;
  if (!in || !out || !in->sequences || !in->slots || !in->textBegins || !in->numOps || !in->ops) return AwFmNullPtrError;
  if ((!text && length != 0) || (!sequenceEnds && numRecords != 0)) return AwFmNullPtrError;
  if ((out->cigarChars && !out->cigarOffsets) || (out->mdChars && !out->mdOffsets)) return AwFmNullPtrError;
  if (numReads >= (1ull << 32) || maxCandidates < 1 || maxCandidates > AWFM_CANDIDATES_MAX_SLOTS) return AwFmIllegalPositionError;
  if (maxOps < 1 || maxOps > AWFM_ALIGN_MAX_OPS || (flags & ~AWFM_STRINGS_CIGAR_M)) return AwFmIllegalPositionError;
  struct awfmStringsCtx ctx;
  memset(&ctx, 0, sizeof ctx);
  ctx.in = in;
  ctx.out = out;
  ctx.text = text;
  ctx.ends = sequenceEnds;
  ctx.length = length;
  ctx.numRecords = numRecords;
  ctx.slots = maxCandidates;
  ctx.maxOps = maxOps;
  ctx.classic = (flags & AWFM_STRINGS_CIGAR_M) != 0;
  ctx.amino = alphabet == AwFmAlphabetAmino;
  ctx.cigarLengths = malloc(numReads * sizeof(uint32_t));
  ctx.mdLengths = malloc(numReads * sizeof(uint32_t));
  ctx.textAt = malloc(numReads * sizeof(uint64_t));
  if (!ctx.cigarLengths || !ctx.mdLengths || !ctx.textAt) {
    free(ctx.cigarLengths);
    free(ctx.mdLengths);
    free(ctx.textAt);
    return AwFmAllocationFailure;
  }
  awfmParallelFor(threads ? threads : 1, numReads, awfmStringsLengthsRange, &ctx);
  if (out->cigarOffsets) {
    uint64_t sum = 0;
    for (uint64_t r = 0; r < numReads; r++) {
      out->cigarOffsets[r] = sum;
      sum += ctx.cigarLengths[r];
    }
    out->cigarOffsets[numReads] = sum;
  }
  if (out->mdOffsets) {
    uint64_t sum = 0;
    for (uint64_t r = 0; r < numReads; r++) {
      out->mdOffsets[r] = sum;
      sum += ctx.mdLengths[r];
    }
    out->mdOffsets[numReads] = sum;
  }
  if (out->cigarChars || out->mdChars) awfmParallelFor(threads ? threads : 1, numReads, awfmStringsWriteRange, &ctx);
  uint64_t skipped = 0, overflow = 0;
  for (unsigned t = 0; t < 64; t++) {
    skipped += ctx.skipped[t];
    overflow += ctx.overflow[t];
  }
  if (out->numSkipped) *out->numSkipped += skipped;
  if (out->numOverflow) *out->numOverflow += overflow;
  free(ctx.cigarLengths);
  free(ctx.mdLengths);
  free(ctx.textAt);
  return AwFmSuccess;
}
