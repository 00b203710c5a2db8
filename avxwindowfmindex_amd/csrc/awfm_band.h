/*
 * awfm_band.h -- what the host twins of the read path share (awfm_verify.c, awfm_align.c, awfm_align_affine.c, awfm_score_affine.c,
 * awfm_window_affine.c): the letter comparison, the arithmetic on "minus infinity", a record's bounds, the classification of a
 * chain slot up to TOO WIDE, the argument checks of the entry points and the rows of the banded affine recurrence, whose diagonal
 * scores by two costs or by a substitution matrix.  The device's
 * definitions of the same things are awfm_band_kernel.h.  Plain C11, static inline and header-only on purpose: a twin is also
 * compiled on its own, by naming its source files.  Exact and readable rather than fast.
 */
#ifndef AWFM_BAND_H
#define AWFM_BAND_H

#include <stddef.h>
#include <stdint.h>

#include "awfm_gpu.h"
#include "awfm_internal.h"

#define AWFM_BAND_NEG INT32_MIN /* minus infinity: awfmBandMinus keeps it what it is */
#define AWFM_SLOT_HAS_BAND 0u   /* what awfmClassifySlot returns for a slot without a status */

/* 0 when both characters map to the same proper letter, one of the twenty or of the four */
static inline uint32_t awfmBandSub(int amino, uint8_t a, uint8_t b) {
  const uint8_t x = amino ? awfmAminoAsciiToIndex(a) : awfmNucAsciiToIndex(a);
  const uint8_t y = amino ? awfmAminoAsciiToIndex(b) : awfmNucAsciiToIndex(b);
  return x == y && x < (amino ? 20u : 4u) ? 0u : 1u;
}

static inline int32_t awfmBandMinus(int32_t value, int32_t cost) { return value == AWFM_BAND_NEG ? AWFM_BAND_NEG : value - cost; }
static inline int32_t awfmBandMax(int32_t a, int32_t b) { return a > b ? a : b; }

/* [*S, *E) of record s < max(numRecords, 1) in the text (numRecords == 0: one sequence [0, length)); 0 when the table does not
 * give it a place inside the text */
static inline int awfmRecordBounds(const uint64_t *ends, uint64_t numRecords, uint64_t length, uint32_t s, uint64_t *S, uint64_t *E) {
  *S = numRecords && s ? ends[s - 1] + 1u : 0u;
  *E = numRecords ? ends[s] : length;
  if (numRecords && s && *S == 0) return 0; /* (an end of 2^64 - 1) */
  return *E >= *S && *E <= length;
}

/* a classified slot that has a band: its record [S, S + L), its read interval and where that begins in the record */
struct awfmSlotBand {
  uint64_t S, rb, re;
  int64_t L, tb, bD, eD;
};

/* Slot `at` (sequence s) of a read of n characters whose offsets are good or not: AWFM_VERIFY_NONE, MALFORMED or TOO_WIDE in the
 * order the header lists the checks, or AWFM_SLOT_HAS_BAND with *b.  The caller goes on with what is its own: TOO LONG, OVERHANG,
 * the band.  0 <= tb <= te <= L < 2^63 and rb, re < 2^32 behind the MALFORMED checks: both diagonals then lie in (-2^32, 2^63)
 * and their difference is taken exactly */
static inline uint32_t awfmClassifySlot(const struct AwFmVerifyInputs *in, const uint64_t *ends, uint64_t numRecords, uint64_t length,
                                        uint32_t maxDrift, uint64_t at, uint64_t n, int readOk, struct awfmSlotBand *b) {
  const uint32_t s = in->sequences[at];
  if (s == AWFM_CANDIDATES_NONE || in->chainAnchors[at] == 0) return AWFM_VERIFY_NONE;
  if (!readOk) return AWFM_VERIFY_MALFORMED;
  const uint64_t rb = in->chainReadBegins[at], re = in->chainReadEnds[at];
  if (rb > re || re > n) return AWFM_VERIFY_MALFORMED;
  if (s >= (numRecords ? numRecords : 1u)) return AWFM_VERIFY_MALFORMED;
  uint64_t S, E;
  if (!awfmRecordBounds(ends, numRecords, length, s, &S, &E)) return AWFM_VERIFY_MALFORMED;
  const int64_t bD = in->chainBeginDiagonals[at], eD = in->chainEndDiagonals[at];
  const __int128 tb = (__int128)rb + bD, te = (__int128)re + eD;
  if (tb < 0 || tb > te || te > (__int128)(E - S)) return AWFM_VERIFY_MALFORMED;
  const __int128 delta = (__int128)eD - bD;
  if (delta > (__int128)maxDrift || delta < -(__int128)maxDrift) return AWFM_VERIFY_TOO_WIDE;
  b->S = S;
  b->rb = rb;
  b->re = re;
  b->L = (int64_t)(E - S);
  b->tb = (int64_t)tb;
  b->bD = bD;
  b->eD = eD;
  return AWFM_SLOT_HAS_BAND;
}

/* what every entry point on chain slots refuses, in this order: a null among the inputs (others: the call's own pointers, 0 when
 * one of them is null), more than 2^32 - 1 reads or a slot count outside 1 .. 16, a band of more than 64 diagonals */
static inline enum AwFmReturnCode awfmBandCheckArguments(const struct AwFmVerifyInputs *in, int others, const uint8_t *text, uint64_t length,
                                                         const uint64_t *sequenceEnds, uint64_t numRecords, uint64_t numReads,
                                                         uint32_t maxCandidates, uint32_t bandPad, uint32_t maxDrift) {
  if (!in || !others || !in->readOffsets || !in->sequences || !in->chainAnchors || !in->chainReadBegins || !in->chainReadEnds ||
      !in->chainBeginDiagonals || !in->chainEndDiagonals)
    return AwFmNullPtrError;
  if ((!in->readChars && in->numReadChars != 0) || (!text && length != 0) || (!sequenceEnds && numRecords != 0)) return AwFmNullPtrError;
  if (numReads >= (1ull << 32) || maxCandidates < 1 || maxCandidates > AWFM_CANDIDATES_MAX_SLOTS) return AwFmIllegalPositionError;
  if ((uint64_t)maxDrift + 2ull * bandPad + 1ull > AWFM_VERIFY_MAX_BAND) return AwFmIllegalPositionError;
  return AwFmSuccess;
}

/* match and gapExtend 1 to 255, mismatch and gapOpen 0 to 255 */
static inline int awfmScoringOk(const struct AwFmAlignScoring *scoring) {
  return !(scoring->match < 1 || scoring->match > 255 || scoring->mismatch > 255 || scoring->gapOpen > 255 || scoring->gapExtend < 1 ||
           scoring->gapExtend > 255);
}

/* the class of a character in a substitution matrix (include/awfm_gpu.h, "substitution matrices"): the letter's index, every
 * byte that is no proper letter -- the sentinel included -- in the last class, 20 or 4 */
static inline uint32_t awfmMatrixClass(int amino, uint8_t c) {
  const uint32_t x = amino ? awfmAminoAsciiToIndex(c) : awfmNucAsciiToIndex(c), other = amino ? 20u : 4u;
  return x < other ? x : other;
}

/* the costs of the affine recurrence as the scoring struct gives them, and the alphabet of the comparison; matrix: NULL, or the
 * AWFM_MATRIX_CLASSES x AWFM_MATRIX_CLASSES substitution scores that take the place of match and mismatch; bonus: "end bonus"'s
 * B, 0 for every call without one */
struct awfmAffineCosts {
  int32_t match, mismatch, open, extend;
  int amino;
  const int8_t *matrix;
  int32_t bonus;
};

static inline struct awfmAffineCosts awfmAffineCostsOf(const struct AwFmAlignScoring *scoring, enum AwFmAlphabetType alphabet) {
  const struct awfmAffineCosts c = {(int32_t)scoring->match, (int32_t)scoring->mismatch, (int32_t)scoring->gapOpen, (int32_t)scoring->gapExtend,
                                    alphabet == AwFmAlphabetAmino, NULL, 0};
  return c;
}

/* gapOpen 0 to 255, gapExtend 1 to 255; every substitution value is legal */
static inline int awfmMatrixScoringOk(const struct AwFmMatrixScoring *scoring) {
  return !(scoring->gapOpen > 255 || scoring->gapExtend < 1 || scoring->gapExtend > 255);
}

static inline struct awfmAffineCosts awfmMatrixCostsOf(const struct AwFmMatrixScoring *scoring, enum AwFmAlphabetType alphabet) {
  const struct awfmAffineCosts c = {0, 0, (int32_t)scoring->gapOpen, (int32_t)scoring->gapExtend, alphabet == AwFmAlphabetAmino,
                                    scoring->substitution, 0};
  return c;
}

/* "end bonus" (include/awfm_gpu.h): the matrix's costs and B, 0 to AWFM_END_BONUS_MAX */
static inline struct awfmAffineCosts awfmEndBonusCostsOf(const struct AwFmMatrixScoring *scoring, uint32_t endBonus, enum AwFmAlphabetType alphabet) {
  struct awfmAffineCosts c = awfmMatrixCostsOf(scoring, alphabet);
  c.bonus = (int32_t)endBonus;
  return c;
}

/* s(a, b) of the recurrence, a of the read and b of the text: the one place the diagonal's score comes from.  sub: verification's */
static inline int32_t awfmAffineDiagonal(const struct awfmAffineCosts *c, uint32_t sub, uint8_t a, uint8_t b) {
  if (c->matrix) return c->matrix[awfmMatrixClass(c->amino, a) * AWFM_MATRIX_CLASSES + awfmMatrixClass(c->amino, b)];
  return sub ? -c->mismatch : c->match;
}

/* a trace byte: the source of H in its low three bits, then whether F and E of the cell open their gap at its neighbour */
enum { AWFM_SRC_STOP = 0, AWFM_SRC_EQ = 1, AWFM_SRC_X = 2, AWFM_SRC_F = 3, AWFM_SRC_E = 4, AWFM_TRACE_F_OPENS = 8, AWFM_TRACE_E_OPENS = 16 };

/* the end cell of a banded local alignment: the largest V over existing cells with i >= 1 -- V is H, and H + bonus for a cell of
 * row n with H > 0 ("end bonus") --, then the smallest i, then the smallest t = i + lo + k; score is that V, 0: there is none */
struct awfmAffineEnd {
  int32_t score;
  int64_t i, k;
};

/* no cell with i >= 1 exists: nothing is aligned, nothing is read */
static inline int awfmAffineNoCell(int64_t n, int64_t L, int64_t lo, int64_t hi) { return n == 0 || n + hi < 0 || lo + 1 > L; }

/* The rows of "affine alignment" as the header states the recurrence: R[0 .. n) against the record T[0 .. L) inside the diagonals
 * [lo, hi] (hi - lo + 1 <= 64, anywhere relative to the record, some cell with i >= 1 exists), three rows of at most 64 cells.
 * trace: NULL, or n x width trace bytes to fill */
static inline struct awfmAffineEnd awfmAffineRows(const struct awfmAffineCosts *c, const uint8_t *R, int64_t n, const uint8_t *T, int64_t L,
                                                  int64_t lo, int64_t hi, uint8_t *trace) {
  int32_t rowsH[2][AWFM_VERIFY_MAX_BAND], rowsF[2][AWFM_VERIFY_MAX_BAND], E[AWFM_VERIFY_MAX_BAND];
  const int64_t width = hi - lo + 1;
  int32_t *prevH = rowsH[0], *curH = rowsH[1], *prevF = rowsF[0], *curF = rowsF[1];
  const int32_t open = c->open + c->extend, extend = c->extend;
  struct awfmAffineEnd end = {0, 0, 0};
  for (int64_t k = 0; k < width; k++) { /* row 0 */
    const int64_t t = lo + k;
    prevH[k] = t >= 0 && t <= L ? c->bonus : AWFM_BAND_NEG;
    prevF[k] = AWFM_BAND_NEG;
  }
  for (int64_t i = 1; i <= n; i++) {
    for (int64_t k = 0; k < width; k++) {
      const int64_t t = i + lo + k;
      uint8_t code = AWFM_SRC_STOP;
      curH[k] = curF[k] = E[k] = AWFM_BAND_NEG;
      if (t >= 0 && t <= L) {
        /* (i-1, t-1) lies on the same diagonal, (i-1, t) on the next one up, (i, t-1) on the one below */
        const uint32_t sub = t >= 1 ? awfmBandSub(c->amino, R[i - 1], T[t - 1]) : 1u;
        const int32_t M = t >= 1 ? awfmBandMinus(prevH[k], -awfmAffineDiagonal(c, sub, R[i - 1], T[t - 1])) : AWFM_BAND_NEG;
        const int32_t fOpens = awfmBandMinus(k + 1 < width ? prevH[k + 1] : AWFM_BAND_NEG, open);
        const int32_t fExtends = awfmBandMinus(k + 1 < width ? prevF[k + 1] : AWFM_BAND_NEG, extend);
        const int32_t eOpens = awfmBandMinus(k >= 1 ? curH[k - 1] : AWFM_BAND_NEG, open);
        const int32_t eExtends = awfmBandMinus(k >= 1 ? E[k - 1] : AWFM_BAND_NEG, extend);
        const int32_t F = awfmBandMax(fOpens, fExtends), e = awfmBandMax(eOpens, eExtends);
        const int32_t H = awfmBandMax(awfmBandMax(0, M), awfmBandMax(F, e));
        curH[k] = H;
        curF[k] = F;
        E[k] = e;
        code = H == 0 ? AWFM_SRC_STOP : M == H ? (sub ? AWFM_SRC_X : AWFM_SRC_EQ) : F == H ? AWFM_SRC_F : AWFM_SRC_E;
        code |= (fOpens >= fExtends ? AWFM_TRACE_F_OPENS : 0) | (eOpens >= eExtends ? AWFM_TRACE_E_OPENS : 0);
        const int32_t V = i == n && H > 0 ? H + c->bonus : H;
        if (V > end.score) { /* rows in ascending order, then columns: the smallest i, then the smallest t of the largest V */
          end.score = V;
          end.i = i;
          end.k = k;
        }
      }
      if (trace) trace[(i - 1) * width + k] = code;
    }
    int32_t *swap = prevH;
    prevH = curH;
    curH = swap;
    swap = prevF;
    prevF = curF;
    curF = swap;
  }
  return end;
}

#endif
