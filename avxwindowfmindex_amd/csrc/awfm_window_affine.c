/*
 * awfm_window_affine.c -- awfmScoreWindowsAffine (include/awfm_gpu.h, "window scores"): the full-width local affine alignment of
 * every read against the text window the caller names, with its begin and end cell and a chain slot.  The host twin of
 * awfmGpuScoreWindowsAffine and its checker: a read at a time, two rows of W + 1 cells with the three values and their origins,
 * the recurrence and the origin rule as the header states them, no n x W table and no walk.  Exact and readable rather than
 * fast.  The reference has no analogue (it stops at positions: ref src/AwFmParallelSearch.c:315-365).
 */
#include <stdlib.h>
#include <string.h>

#include "awfm_band.h"

struct awfmWindowCtx {
  const struct AwFmWindowInputs *in;
  const struct AwFmWindowOutputs *out;
  const uint8_t *text;
  const uint64_t *ends;
  uint64_t length, numRecords;
  uint32_t stride, column, floor;
  int32_t match, mismatch, open, extend;
  int amino, failed;
  uint64_t unscored[64], found[64]; /* per thread of the loop */
};

/* a cell: the three values, and where the path behind each of them began */
struct awfmWindowCell {
  int32_t H, E, F;
  uint32_t hI, hT, eI, eT, fI, fT;
};

struct awfmWindowResult {
  uint32_t value, readBegin, readEnd; /* value: a score or a status */
  uint64_t textBegin, textEnd;        /* window-local until the caller adds b */
};

/* R[0 .. n) against T[0 .. W), every cell: the largest H with i >= 1, then the smallest i, then the smallest t, and its origin */
static void awfmWindowRead(const struct awfmWindowCtx *c, const uint8_t *R, uint32_t n, const uint8_t *T, uint32_t W,
                           struct awfmWindowCell *prev, struct awfmWindowCell *cur, struct awfmWindowResult *a) {
  const int32_t open = c->open + c->extend, extend = c->extend;
  for (uint32_t t = 0; t <= W; t++) { /* row 0 */
    prev[t].H = 0;
    prev[t].E = prev[t].F = AWFM_BAND_NEG;
    prev[t].hI = 0;
    prev[t].hT = t;
    prev[t].eI = prev[t].eT = prev[t].fI = prev[t].fT = 0;
  }
  int32_t best = 0;
  for (uint32_t i = 1; i <= n; i++) {
    for (uint32_t t = 0; t <= W; t++) {
      struct awfmWindowCell *x = &cur[t];
      const struct awfmWindowCell *up = &prev[t];
      const int32_t M = t >= 1 ? prev[t - 1].H + (awfmBandSub(c->amino, R[i - 1], T[t - 1]) ? -c->mismatch : c->match) : AWFM_BAND_NEG;
      const int32_t fOpens = up->H - open, fExtends = awfmBandMinus(up->F, extend);
      x->F = fOpens >= fExtends ? fOpens : fExtends;
      x->fI = fOpens >= fExtends ? up->hI : up->fI;
      x->fT = fOpens >= fExtends ? up->hT : up->fT;
      x->E = AWFM_BAND_NEG;
      x->eI = x->eT = 0;
      if (t >= 1) {
        const struct awfmWindowCell *left = &cur[t - 1];
        const int32_t eOpens = left->H - open, eExtends = awfmBandMinus(left->E, extend);
        x->E = eOpens >= eExtends ? eOpens : eExtends;
        x->eI = eOpens >= eExtends ? left->hI : left->eI;
        x->eT = eOpens >= eExtends ? left->hT : left->eT;
      }
      int32_t H = 0;
      if (M > H) H = M;
      if (x->F > H) H = x->F;
      if (x->E > H) H = x->E;
      x->H = H;
      if (H == 0) {
        x->hI = i;
        x->hT = t;
      } else if (M == H) {
        x->hI = prev[t - 1].hI;
        x->hT = prev[t - 1].hT;
      } else if (x->F == H) {
        x->hI = x->fI;
        x->hT = x->fT;
      } else {
        x->hI = x->eI;
        x->hT = x->eT;
      }
      if (H > best) { /* rows in ascending order, then columns: the smallest i, then the smallest t of the largest H */
        best = H;
        a->readEnd = i;
        a->textEnd = t;
        a->readBegin = x->hI;
        a->textBegin = x->hT;
      }
    }
    struct awfmWindowCell *swap = prev;
    prev = cur;
    cur = swap;
  }
  a->value = (uint32_t)best;
}

/* the two rows of a thread's loop: they grow to the widest window the thread meets and are freed when its range is done */
struct awfmWindowRows {
  struct awfmWindowCell *cells;
  uint64_t width; /* cells per row */
};

/* 0 when the rows could not be had */
static int awfmWindowOne(const struct awfmWindowCtx *c, uint64_t r, struct awfmWindowRows *rows, struct awfmWindowResult *a) {
  const struct AwFmWindowInputs *in = c->in;
  const uint32_t s = in->windowSequences[r];
  memset(a, 0, sizeof *a);
  a->value = AWFM_VERIFY_MALFORMED;
  if (s >= (c->numRecords ? c->numRecords : 1u)) return 1;
  const uint64_t begin = in->windowBegins[r], end = in->windowEnds[r];
  if (begin > end) return 1;
  const uint64_t readBegin = in->readOffsets[r], readEnd = in->readOffsets[r + 1];
  if (readBegin > readEnd || readEnd > in->numReadChars) return 1;
  uint64_t S, E;
  if (!awfmRecordBounds(c->ends, c->numRecords, c->length, s, &S, &E)) return 1;
  const uint64_t L = E - S, b = begin < L ? begin : L, e = end < L ? end : L, W = e - b, n = readEnd - readBegin;
  if (W > AWFM_WINDOW_MAX_WIDTH) {
    a->value = AWFM_VERIFY_TOO_WIDE;
    return 1;
  }
  if (n > AWFM_WINDOW_MAX_LENGTH) {
    a->value = AWFM_VERIFY_TOO_LONG;
    return 1;
  }
  a->value = 0;
  if (n == 0 || W == 0) return 1; /* nothing is aligned, nothing is read */
  if (rows->width < W + 1u) {
    struct awfmWindowCell *cells = realloc(rows->cells, 2u * (W + 1u) * sizeof *cells);
    if (!cells) return 0;
    rows->cells = cells;
    rows->width = W + 1u;
  }
  awfmWindowRead(c, in->readChars + readBegin, (uint32_t)n, c->text + S + b, (uint32_t)W, rows->cells, rows->cells + rows->width, a);
  if (a->value == 0) return 1;
  a->textBegin += b;
  a->textEnd += b;
  return 1;
}

static void awfmWindowRange(void *p, uint64_t begin, uint64_t end, unsigned tid) {
  struct awfmWindowCtx *c = p;
  const struct AwFmWindowOutputs *out = c->out;
  struct awfmWindowRows rows = {NULL, 0};
  uint64_t unscored = 0, found = 0;
  for (uint64_t r = begin; r < end; r++) {
    struct awfmWindowResult a;
    const int looked = c->in->windowSequences[r] != AWFM_CANDIDATES_NONE;
    if (looked) {
      if (!awfmWindowOne(c, r, &rows, &a)) {
        c->failed = 1;
        break;
      }
    } else {
      memset(&a, 0, sizeof a);
      a.value = AWFM_VERIFY_NONE;
    }
    if (out->scores) out->scores[r] = a.value;
    if (out->readBegins) out->readBegins[r] = a.readBegin;
    if (out->readEnds) out->readEnds[r] = a.readEnd;
    if (out->textBegins) out->textBegins[r] = a.textBegin;
    if (out->textEnds) out->textEnds[r] = a.textEnd;
    if (!looked) continue;
    if (a.value >= AWFM_VERIFY_TOO_LONG) unscored++;
    const int counts = a.value < AWFM_VERIFY_TOO_LONG && a.value >= c->floor;
    found += (uint64_t)counts;
    const uint64_t at = r * c->stride + c->column;
    if (out->sequences) out->sequences[at] = counts ? c->in->windowSequences[r] : AWFM_CANDIDATES_NONE;
    if (out->chainAnchors) out->chainAnchors[at] = counts ? 1u : 0u;
    if (out->chainReadBegins) out->chainReadBegins[at] = counts ? a.readBegin : 0u;
    if (out->chainReadEnds) out->chainReadEnds[at] = counts ? a.readEnd : 0u;
    if (out->chainBeginDiagonals) out->chainBeginDiagonals[at] = counts ? (int64_t)a.textBegin - (int64_t)a.readBegin : 0;
    if (out->chainEndDiagonals) out->chainEndDiagonals[at] = counts ? (int64_t)a.textEnd - (int64_t)a.readEnd : 0;
  }
  free(rows.cells);
  c->unscored[tid & 63u] += unscored;
  c->found[tid & 63u] += found;
}

enum AwFmReturnCode awfmScoreWindowsAffine(const struct AwFmWindowInputs *in, uint64_t numReads, const struct AwFmAlignScoring *scoring,
                                           uint32_t minScore, uint32_t slotStride, uint32_t slotColumn, const uint8_t *text, uint64_t length,
                                           const uint64_t *sequenceEnds, uint64_t numRecords, enum AwFmAlphabetType alphabet,
                                           const struct AwFmWindowOutputs *out, unsigned threads) {
  if (numReads == 0) return AwFmSuccess;
  if (!in || !out || !scoring || !in->readOffsets || !in->windowSequences || !in->windowBegins || !in->windowEnds) return AwFmNullPtrError;
  if ((!in->readChars && in->numReadChars != 0) || (!text && length != 0) || (!sequenceEnds && numRecords != 0)) return AwFmNullPtrError;
  if (numReads >= (1ull << 32) || slotStride < 1 || slotStride > AWFM_CANDIDATES_MAX_SLOTS || slotColumn >= slotStride)
    return AwFmIllegalPositionError;
  if (!awfmScoringOk(scoring)) return AwFmIllegalPositionError;
  struct awfmWindowCtx ctx;
  memset(&ctx, 0, sizeof ctx);
  ctx.in = in;
  ctx.out = out;
  ctx.text = text;
  ctx.ends = sequenceEnds;
  ctx.length = length;
  ctx.numRecords = numRecords;
  ctx.stride = slotStride;
  ctx.column = slotColumn;
  ctx.floor = minScore > 1u ? minScore : 1u;
  ctx.match = (int32_t)scoring->match;
  ctx.mismatch = (int32_t)scoring->mismatch;
  ctx.open = (int32_t)scoring->gapOpen;
  ctx.extend = (int32_t)scoring->gapExtend;
  ctx.amino = alphabet == AwFmAlphabetAmino;
  awfmParallelFor(threads ? threads : 1, numReads, awfmWindowRange, &ctx);
  if (ctx.failed) return AwFmAllocationFailure;
  uint64_t unscored = 0, found = 0;
  for (unsigned t = 0; t < 64; t++) {
    unscored += ctx.unscored[t];
    found += ctx.found[t];
  }
  if (out->numUnscored) *out->numUnscored += unscored;
  if (out->numFound) *out->numFound += found;
  return AwFmSuccess;
}
