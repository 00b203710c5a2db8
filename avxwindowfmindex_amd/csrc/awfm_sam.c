/*
 * awfm_sam.c -- awfmSamRecords (include/awfm_gpu.h, "SAM records"): one SAM line per read, packed behind offsets.  The host twin
 * of awfmGpuSamRecords and its checker: a read at a time, the header's rules as written.  ONE formatter both counts and writes
 * (dst == NULL: count), so a length and the bytes behind it cannot disagree.  Three passes: the lengths over `threads` threads,
 * the prefix sums on one, the bytes over `threads` threads.  Exact and readable rather than fast.  Also the two host-only
 * helpers that need the index: awfmRecordNames and awfmSamHeader.  The reference has no analogue.
 */
#include <stdlib.h>
#include <string.h>

#include "awfm_gpu.h"
#include "awfm_internal.h"

/* `value` in decimal without leading zeros at dst + at (dst == NULL: nothing is stored); returns where it ends */
static uint64_t awfmSamDecimal(uint8_t *dst, uint64_t at, uint64_t value) {
  unsigned digits = 1;
  for (uint64_t v = value; v >= 10u; v /= 10u) digits++;
  if (dst) {
    uint64_t v = value;
    for (unsigned d = digits; d > 0; d--, v /= 10u) dst[at + d - 1u] = (uint8_t)('0' + v % 10u);
  }
  return at + digits;
}

static uint64_t awfmSamByte(uint8_t *dst, uint64_t at, uint8_t c) {
  if (dst) dst[at] = c;
  return at + 1u;
}

static uint64_t awfmSamBytes(uint8_t *dst, uint64_t at, const uint8_t *src, uint64_t length) {
  if (dst && length) memcpy(dst + at, src, length);
  return at + length;
}

/* the bytes, or `*` when there are none */
static uint64_t awfmSamBytesOrStar(uint8_t *dst, uint64_t at, const uint8_t *src, uint64_t length) {
  return length ? awfmSamBytes(dst, at, src, length) : awfmSamByte(dst, at, '*');
}

static uint64_t awfmSamTag(uint8_t *dst, uint64_t at, const char *tag) { /* a tab and the five characters of "XX:t:" */
  return awfmSamBytes(dst, awfmSamByte(dst, at, '\t'), (const uint8_t *)tag, 5);
}

struct awfmSamCtx {
  const struct AwFmSamInputs *in;
  const struct AwFmSamOutputs *out;
  uint64_t numReads;
  uint32_t slots;
  int paired;
  uint32_t *lengths;                    /* [numReads] */
  uint64_t unaligned[64], overflow[64]; /* per thread of the loop */
};

/* ALIGNED or not, by the header's list; *s: the record */
static int awfmSamIsAligned(const struct awfmSamCtx *c, uint64_t r, uint32_t *s) {
  const struct AwFmSamInputs *in = c->in;
  if (in->scores[r] == 0 || in->scores[r] >= AWFM_VERIFY_TOO_LONG) return 0;
  const uint32_t j = in->slots[r];
  if (j >= c->slots) return 0;
  *s = in->sequences[r * c->slots + j];
  if (*s >= in->numRecordNames) return 0;
  return in->readOffsets[r + 1u] >= in->readOffsets[r];
}

static uint64_t awfmSamRecordName(const struct AwFmSamInputs *in, uint8_t *dst, uint64_t at, uint32_t s) {
  return awfmSamBytes(dst, at, in->recordNameChars + in->recordNameOffsets[s], in->recordNameOffsets[s + 1u] - in->recordNameOffsets[s]);
}

/* the line of read r at dst (NULL: counted only); returns its length */
static uint64_t awfmSamLine(const struct awfmSamCtx *c, uint64_t r, uint8_t *dst) {
  const struct AwFmSamInputs *in = c->in;
  const uint64_t m = r ^ 1u;
  uint32_t s = 0, sm = 0;
  const int aligned = awfmSamIsAligned(c, r, &s), mateAligned = c->paired && awfmSamIsAligned(c, m, &sm);
  const uint64_t n = in->readOffsets[r + 1u] >= in->readOffsets[r] ? in->readOffsets[r + 1u] - in->readOffsets[r] : 0u;
  uint64_t at = 0;
  /* QNAME */
  if (in->nameOffsets) at = awfmSamBytes(dst, at, in->nameChars + in->nameOffsets[r], in->nameOffsets[r + 1u] - in->nameOffsets[r]);
  else at = awfmSamDecimal(dst, at, c->paired ? r / 2u : r);
  /* FLAG */
  uint32_t flag = in->baseFlags ? in->baseFlags[r] : 0u;
  if (!aligned) flag |= 0x4u;
  if (c->paired) {
    flag |= 0x1u | ((r & 1u) ? 0x80u : 0x40u);
    if (in->properPairs && in->properPairs[r / 2u] && aligned && mateAligned) flag |= 0x2u;
    if (!mateAligned) flag |= 0x8u;
    if (in->baseFlags && (in->baseFlags[m] & 0x10u)) flag |= 0x20u;
  }
  at = awfmSamDecimal(dst, awfmSamByte(dst, at, '\t'), flag);
  /* RNAME, POS: the read's own place, or the aligned mate's */
  const int placed = aligned || mateAligned;
  const uint32_t place = aligned ? s : sm;
  at = awfmSamByte(dst, at, '\t');
  at = placed ? awfmSamRecordName(in, dst, at, place) : awfmSamByte(dst, at, '*');
  at = awfmSamDecimal(dst, awfmSamByte(dst, at, '\t'), placed ? in->textBegins[aligned ? r : m] + 1u : 0u);
  /* MAPQ */
  at = awfmSamDecimal(dst, awfmSamByte(dst, at, '\t'), aligned ? (in->mappingQualities ? in->mappingQualities[r] : 255u) : 0u);
  /* CIGAR */
  at = awfmSamByte(dst, at, '\t');
  at = awfmSamBytesOrStar(dst, at, in->cigarChars + in->cigarOffsets[r], aligned ? in->cigarOffsets[r + 1u] - in->cigarOffsets[r] : 0u);
  /* RNEXT, PNEXT */
  at = awfmSamByte(dst, at, '\t');
  if (!mateAligned) at = awfmSamByte(dst, at, '*');
  else if (place == sm) at = awfmSamByte(dst, at, '=');
  else at = awfmSamRecordName(in, dst, at, sm);
  at = awfmSamDecimal(dst, awfmSamByte(dst, at, '\t'), mateAligned ? in->textBegins[m] + 1u : 0u);
  /* TLEN */
  at = awfmSamByte(dst, at, '\t');
  uint64_t span = 0;
  int negative = 0;
  if (aligned && mateAligned && s == sm) {
    const uint64_t b = in->textBegins[r] < in->textBegins[m] ? in->textBegins[r] : in->textBegins[m];
    const uint64_t e = in->textEnds[r] > in->textEnds[m] ? in->textEnds[r] : in->textEnds[m];
    const int first = in->textBegins[r] < in->textBegins[m] || (in->textBegins[r] == in->textBegins[m] && (r & 1u) == 0u);
    span = first ? e - b : 0u - (e - b); /* 64-bit two's complement */
    negative = (span >> 63) != 0;
  }
  if (negative) at = awfmSamByte(dst, at, '-');
  at = awfmSamDecimal(dst, at, negative ? 0u - span : span);
  /* SEQ, QUAL */
  at = awfmSamBytesOrStar(dst, awfmSamByte(dst, at, '\t'), in->readChars + in->readOffsets[r], n);
  at = awfmSamBytesOrStar(dst, awfmSamByte(dst, at, '\t'), in->qualities ? in->qualities + in->readOffsets[r] : NULL, in->qualities ? n : 0u);
  /* tags */
  if (aligned) {
    at = awfmSamDecimal(dst, awfmSamTag(dst, at, "NM:i:"), in->editDistances[r]);
    at = awfmSamDecimal(dst, awfmSamTag(dst, at, "AS:i:"), in->scores[r]);
    if (in->secondScores) at = awfmSamDecimal(dst, awfmSamTag(dst, at, "XS:i:"), in->secondScores[r]);
    if (in->mdOffsets && in->mdOffsets[r + 1u] != in->mdOffsets[r])
      at = awfmSamBytes(dst, awfmSamTag(dst, at, "MD:Z:"), in->mdChars + in->mdOffsets[r], in->mdOffsets[r + 1u] - in->mdOffsets[r]);
  }
  return awfmSamByte(dst, at, '\n');
}

static void awfmSamLengthsRange(void *ctx, uint64_t begin, uint64_t end, unsigned tid) {
  struct awfmSamCtx *c = ctx;
  uint64_t unaligned = 0;
  for (uint64_t r = begin; r < end; r++) {
    uint32_t s;
    unaligned += !awfmSamIsAligned(c, r, &s);
    c->lengths[r] = (uint32_t)awfmSamLine(c, r, NULL);
  }
  c->unaligned[tid & 63u] += unaligned;
}

static void awfmSamWriteRange(void *ctx, uint64_t begin, uint64_t end, unsigned tid) {
  struct awfmSamCtx *c = ctx;
  const struct AwFmSamOutputs *out = c->out;
  uint64_t overflow = 0;
  for (uint64_t r = begin; r < end; r++) {
    if (out->lineOffsets[r + 1u] <= out->lineCapacity) awfmSamLine(c, r, out->lineChars + out->lineOffsets[r]);
    else overflow++;
  }
  c->overflow[tid & 63u] += overflow;
}

enum AwFmReturnCode awfmSamRecords(const struct AwFmSamInputs *in, uint64_t numReads, uint32_t maxCandidates, uint32_t flags,
                                   const struct AwFmSamOutputs *out, unsigned threads) {
  if (numReads == 0) return AwFmSuccess;
  if (!in || !out || !in->readChars || !in->readOffsets || !in->sequences || !in->slots || !in->scores || !in->editDistances ||
      !in->textBegins || !in->textEnds || !in->cigarOffsets || !in->cigarChars)
    return AwFmNullPtrError;
  if (in->numRecordNames != 0 && (!in->recordNameOffsets || !in->recordNameChars)) return AwFmNullPtrError;
  if (!in->nameOffsets != !in->nameChars || !in->mdOffsets != !in->mdChars) return AwFmNullPtrError;
  if (out->lineChars && !out->lineOffsets) return AwFmNullPtrError;
  if (maxCandidates < 1 || maxCandidates > AWFM_CANDIDATES_MAX_SLOTS || (flags & ~AWFM_SAM_PAIRED)) return AwFmIllegalPositionError;
  if (((flags & AWFM_SAM_PAIRED) && (numReads & 1u)) || numReads >= (1ull << 32)) return AwFmIllegalPositionError;
  struct awfmSamCtx ctx;
  memset(&ctx, 0, sizeof ctx);
  ctx.in = in;
  ctx.out = out;
  ctx.numReads = numReads;
  ctx.slots = maxCandidates;
  ctx.paired = (flags & AWFM_SAM_PAIRED) != 0;
  ctx.lengths = malloc(numReads * sizeof(uint32_t));
  if (!ctx.lengths) return AwFmAllocationFailure;
  awfmParallelFor(threads ? threads : 1, numReads, awfmSamLengthsRange, &ctx);
  if (out->lineOffsets) {
    uint64_t sum = 0;
    for (uint64_t r = 0; r < numReads; r++) {
      out->lineOffsets[r] = sum;
      sum += ctx.lengths[r];
    }
    out->lineOffsets[numReads] = sum;
  }
  if (out->lineChars) awfmParallelFor(threads ? threads : 1, numReads, awfmSamWriteRange, &ctx);
  uint64_t unaligned = 0, overflow = 0;
  for (unsigned t = 0; t < 64; t++) {
    unaligned += ctx.unaligned[t];
    overflow += ctx.overflow[t];
  }
  if (out->numUnaligned) *out->numUnaligned += unaligned;
  if (out->numOverflow) *out->numOverflow += overflow;
  free(ctx.lengths);
  return AwFmSuccess;
}

/* the first whitespace-delimited token of record i's header */
static const uint8_t *awfmSamRecordToken(const struct FastaVector *fv, size_t i, uint64_t *length) {
  const size_t begin = i == 0 ? 0 : fv->records[i - 1u].headerEndPosition, end = fv->records[i].headerEndPosition;
  size_t from = begin, to;
  while (from < end && (fv->headers[from] == ' ' || (fv->headers[from] >= '\t' && fv->headers[from] <= '\r'))) from++;
  for (to = from; to < end && !(fv->headers[to] == ' ' || (fv->headers[to] >= '\t' && fv->headers[to] <= '\r')); to++) {
  }
  *length = to - from;
  return (const uint8_t *)fv->headers + from;
}

enum AwFmReturnCode awfmRecordNames(const struct AwFmIndex *index, uint64_t *offsets, uint8_t *chars, uint64_t capacity) {
  if (!index || !offsets) return AwFmNullPtrError;
  const struct FastaVector *fv = index->fastaVector;
  if (!fv) return AwFmUnsupportedVersionError;
  uint64_t at = 0;
  for (size_t i = 0; i < fv->numRecords; i++) {
    uint64_t length;
    const uint8_t *token = awfmSamRecordToken(fv, i, &length);
    offsets[i] = at;
    if (chars && at + length <= capacity && length) memcpy(chars + at, token, length);
    at += length;
  }
  offsets[fv->numRecords] = at;
  return AwFmSuccess;
}

uint64_t awfmSamHeader(const struct AwFmIndex *index, uint8_t *out, uint64_t capacity) {
  static const char first[] = "@HD\tVN:1.6\tSO:unknown\n";
  const struct FastaVector *fv = index ? index->fastaVector : NULL;
  if (!fv || fv->numRecords == 0) return 0;
  uint64_t at = sizeof first - 1u;
  if (out && at <= capacity) memcpy(out, first, at);
  for (size_t i = 0; i < fv->numRecords; i++) {
    uint64_t length;
    const uint8_t *token = awfmSamRecordToken(fv, i, &length);
    const uint64_t begin = i == 0 ? 0 : (uint64_t)fv->records[i - 1u].sequenceEndPosition + 1u;
    const uint64_t residues = (uint64_t)fv->records[i].sequenceEndPosition - begin;
    const uint64_t end = awfmSamDecimal(NULL, at + 7u + length + 4u, residues) + 1u;
    uint8_t *dst = out && end <= capacity ? out : NULL; /* a line is written whole or not at all */
    at = awfmSamBytes(dst, at, (const uint8_t *)"@SQ\tSN:", 7);
    at = awfmSamBytes(dst, at, token, length);
    at = awfmSamBytes(dst, at, (const uint8_t *)"\tLN:", 4);
    at = awfmSamByte(dst, awfmSamDecimal(dst, at, residues), '\n');
  }
  return at;
}
